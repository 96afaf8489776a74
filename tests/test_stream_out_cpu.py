"""The outbound loop on the host (`staging.stream_out` with a `cpu` device): device buffer -> two alternating host buffers -> the
caller's writer threads.  Fake producers fill the buffer with the batch's number, fake consumers hand the bytes to a thread pool.
Items of 8 bytes, 2 per batch, 5 items: three batches, the smallest run in which a buffer is used a second time."""
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from globalegomocap_amd import staging

ITEM, PER = 8, 2
NBYTES = ITEM * PER


class Rig:
    """A producer and a consumer that record what happens to them.  `job(k, data)` is what batch k's future runs (default: copy the
    bytes); `fail_at`: the `produce` that raises; `stop_at`: the `consume` that returns STOP."""

    def __init__(self, pool, items=5, job=None, fail_at=None, stop_at=None):
        self.pool, self.items, self.job, self.fail_at, self.stop_at = pool, items, job, fail_at, stop_at
        self.batches = (items + PER - 1) // PER
        self.log, self.futures, self.got, self.sides, self.pointers = [], {}, {}, {}, set()

    def produce(self, k, out):
        self.log.append(("produce", k))
        self.pointers.add(("device", out.data_ptr(), out.numel()))
        if k == self.fail_at:
            raise RuntimeError("producer %d" % k)
        n = min(PER, self.items - k * PER) * ITEM
        out[:n] = k
        return n

    def consume(self, k, data, side):
        self.log.append(("consume", k))
        self.pointers.add(("host", data.data_ptr() if data.numel() <= NBYTES else 0, k % 2))
        if side is not None:
            self.sides[k] = side.view(torch.int64).tolist()
        if k == self.stop_at:
            return staging.STOP
        self.futures[k] = self.pool.submit(self.job or self.keep, k, data)
        return [self.futures[k]]

    def keep(self, k, data):
        self.got[k] = bytes(data.numpy())

    def run(self, key="test", nbytes=NBYTES, produce=None, **kw):
        staging.stream_out("cpu", key, nbytes, self.batches, produce or self.produce, self.consume, **kw)

    def settled(self):
        return all(f.done() for f in self.futures.values())          # (a cancelled future is done)


@pytest.fixture
def pool():
    with ThreadPoolExecutor(max_workers=2) as p:
        yield p
    staging.release_kept("test")


def test_content_and_order(pool):
    r = Rig(pool)
    r.run()
    assert r.got == {0: bytes([0]) * 16, 1: bytes([1]) * 16, 2: bytes([2]) * 8}
    assert r.log == [("produce", 0), ("produce", 1), ("consume", 0), ("produce", 2), ("consume", 1), ("consume", 2)]
    for k in range(r.batches - 1):          # batch k is handed over once batch k + 1 has been enqueued; the last one behind the last produce
        assert r.log.index(("consume", k)) == r.log.index(("produce", k + 1)) + 1
    assert r.log[-1] == ("consume", 2) and r.settled()


def test_a_buffer_is_settled_before_it_is_used_again(pool):
    gate, seen = threading.Event(), {}

    def job(k, data):
        if k == 0:
            gate.wait()
        r.keep(k, data)
        seen["left", k] = True

    r = Rig(pool, job=job)

    def produce(k, out):
        if k == 2:
            seen["batch 0 done before produce(2)"] = r.futures[0].done() and seen.get(("left", 0), False)
        return r.produce(k, out)

    timer = threading.Timer(0.05, gate.set)
    timer.start()
    try:
        r.run(produce=produce)
    finally:
        gate.set()
        timer.cancel()
    assert seen["batch 0 done before produce(2)"] is True
    assert r.got == {0: bytes([0]) * 16, 1: bytes([1]) * 16, 2: bytes([2]) * 8}


def test_a_writers_error_surfaces_and_leaves_nothing_behind(pool):
    def job(k, data):
        if k == 0:
            raise OSError("disk")
        r.keep(k, data)

    r = Rig(pool, job=job)
    with pytest.raises(OSError, match="disk"):
        r.run()
    assert r.settled() and set(r.futures) == {0}
    assert [k for what, k in r.log if what == "produce"] == [0, 1]          # buffer 0 held the failed batch: produce(2) never ran


@pytest.mark.parametrize("fail_at", [1, 3])
def test_a_producers_error_surfaces_and_leaves_nothing_behind(pool, fail_at):
    r = Rig(pool, items=7, fail_at=fail_at)
    with pytest.raises(RuntimeError, match="producer %d" % fail_at):
        r.run()
    assert r.settled() and set(r.futures) == set(range(fail_at - 1))          # (batch fail_at - 1 was enqueued, never handed over)
    assert [k for what, k in r.log if what == "produce"] == list(range(fail_at + 1))


def test_an_error_among_many_writers_cancels_or_awaits_the_others(pool):
    """One batch, many files: the first writer fails while the second is under way and the others have not started."""
    gate, started, finished, futures = threading.Event(), [], [], []

    def job(i):
        if i == 0:
            raise OSError("disk")
        started.append(i)
        gate.wait()
        finished.append(i)

    def consume(k, data, side):
        futures.extend(pool.submit(job, i) for i in range(4 * k, 4 * k + 4))
        return futures[-4:]

    r = Rig(pool)
    timer = threading.Timer(0.05, gate.set)
    timer.start()
    try:
        with pytest.raises(OSError, match="disk"):
            staging.stream_out("cpu", "test", NBYTES, r.batches, r.produce, consume)
        assert len(futures) == 4 and all(f.done() for f in futures) and sorted(started) == sorted(finished)
    finally:
        gate.set()
        timer.cancel()


def test_a_consumer_that_fails_halfway_leaves_nothing_behind(pool):
    """The consumer hands its futures over as a generator and raises after the second: the two are still cancelled or awaited."""
    gate, started, finished, futures = threading.Event(), [], [], []

    def job(i):
        started.append(i)
        gate.wait()
        finished.append(i)

    def consume(k, data, side):
        for i in range(2):
            futures.append(pool.submit(job, i))
            yield futures[-1]
        raise ValueError("consumer")

    r = Rig(pool)
    timer = threading.Timer(0.05, gate.set)
    timer.start()
    try:
        with pytest.raises(ValueError, match="consumer"):
            staging.stream_out("cpu", "test", NBYTES, r.batches, r.produce, consume)
        assert len(futures) == 2 and all(f.done() for f in futures) and sorted(started) == sorted(finished)
    finally:
        gate.set()
        timer.cancel()


def test_stop_ends_the_loop_early(pool):
    r = Rig(pool, items=7, stop_at=1)
    r.run()
    # batch 2 was enqueued before batch 1 was handed over: it is produced and dropped; batch 3 never starts
    assert r.log == [("produce", 0), ("produce", 1), ("consume", 0), ("produce", 2), ("consume", 1)]
    assert r.settled() and r.got == {0: bytes([0]) * 16}


def test_variable_and_oversize_batches(pool):
    r = Rig(pool)
    own = (torch.arange(2 * NBYTES) % 251).to(torch.uint8)

    def produce(k, out):
        n = r.produce(k, out)
        return 5 if k == 0 else own if k == 1 else n

    r.run(produce=produce)
    assert r.got == {0: bytes([0]) * 5, 1: bytes(own.numpy()), 2: bytes([2]) * 8}
    assert [k for what, k in r.log if what == "consume"] == [0, 1, 2]


def test_side_bytes_travel_with_their_batch(pool):
    r = Rig(pool)
    r.run(produce=lambda k, out: (r.produce(k, out), torch.tensor([k, 100 + k], dtype=torch.int64)), side_bytes=16)
    assert r.sides == {0: [0, 100], 1: [1, 101], 2: [2, 102]}
    assert r.got == {0: bytes([0]) * 16, 1: bytes([1]) * 16, 2: bytes([2]) * 8}


def test_buffers_are_kept_remade_and_released(pool):
    first, again, other = Rig(pool), Rig(pool), Rig(pool)
    first.run()
    again.run()
    assert first.pointers == again.pointers and len(first.pointers) == 3          # one device buffer, two host buffers, the same ones
    kept = {k: v for k, v in staging._kept.items() if k[1] == "test"}
    assert sorted(k[2] for k in kept) == ["device", "host0", "host1"] and all(v.numel() == NBYTES for v in kept.values())
    other.run(nbytes=2 * NBYTES)
    assert {p[2] for p in other.pointers if p[0] == "device"} == {2 * NBYTES}
    remade = {k: v for k, v in staging._kept.items() if k[1] == "test"}
    assert sorted(remade) == sorted(kept) and all(v.numel() == 2 * NBYTES and v is not kept[k] for k, v in remade.items())
    assert other.got == first.got
    staging.release()
    assert not staging._kept
