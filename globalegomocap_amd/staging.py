"""How bytes get to the device and back out to files: reader threads next to the device, two copy streams, pinned staging
buffers, and the one two-slot loop device buffer -> pinned memory -> writer threads -> files.

Nothing here knows about chunks, windows, MAT files or file formats.  `whole_sequence` (chunk pickles) and `prepare` (the pose
network's .mat files) are built on the inbound half, the writers (`meshes`, `render`, `bvh`, `video`) on the outbound half:

  * `reader_pool`: the process's named pools of reader threads, optionally confined to the CPUs `cpus_near` the device;
  * `copy_stream` / `report_stream`: the few streams the copies and the read-backs run on;
  * `thread_state` / `staging_buffer`: a reader thread's two alternating pinned buffers and the events that guard them;
  * `Scratch`: a pinned block from which small arrays go up asynchronously;
  * `stream_out` / `kept_bytes` / `release_kept`: the outbound loop and the buffers it keeps between calls;
  * `padded`, `side_by_side`, `natural_key`, `Laps`, `drain`: layout, ordering, timing and clean-up helpers;
  * `release`: gives back what the module keeps between calls.
"""
import os
import re
import threading
import time

import numpy as np
import torch

# Two copy streams per device (one and eight were both slower than two; stream priorities had no effect, so
# the streams are created with the default one).
N_COPY_STREAMS = 2

_pools = {}
_copy_streams = {}
_report_streams = {}
_copy_lock = threading.Lock()
_kept = {}                             # (device, key, part) -> a uint8 buffer kept between calls (`kept_bytes`)
STOP = "stop"                          # what a `stream_out` consumer returns to end the loop early
_reader_local = threading.local()      # per reader thread: two pinned staging buffers, (whole_sequence.load_chunk only) a device image of the file


def natural_key(name):
    """Sort key equivalent to natsort.natsorted (default algorithm: case-sensitive text, unsigned integers) for directory
    names like chunk_2 < chunk_10 (optimize_whole_sequence.py:48)."""
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def padded(nbytes, align):
    """Room for `nbytes` plus at least 8 bytes of slack, on an `align`-byte boundary (the device readers take whole words, which
    may reach past a payload's last byte).  Works on ints and on numpy arrays of them."""
    return (nbytes + 8 + align - 1) // align * align


def side_by_side(sizes, align):
    """Files of `sizes` bytes laid out side by side in one block: (at, room, total) -- file i lies at at[i] and has room[i] =
    padded(sizes[i], align) bytes to itself."""
    room = padded(np.asarray(sizes, dtype=np.int64), align)
    return np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64), room, int(room.sum())


class Laps:
    """Developer timing of the calling thread's phases: `lap(name)` adds the wall time since the last lap to `timings[name]`
    (a caller-supplied dict, None = nothing is measured).  With `log`, every lap is also appended to `timings["_log"]` as
    (ms since this object was made, name)."""

    def __init__(self, timings, log=False):
        self.timings, self.log = timings, log
        self.begin = self.tick = time.perf_counter()

    def __call__(self, name):
        if self.timings is None:
            return
        now = time.perf_counter()
        self.timings[name] = self.timings.get(name, 0.0) + (now - self.tick)
        if self.log:
            self.timings.setdefault("_log", []).append((round((now - self.begin) * 1e3, 2), name))
        self.tick = now


def cpus_near(device):
    """The CPUs of the NUMA node the device hangs off (its PCIe root), as far as this process may run on them -- or None when
    the platform does not say.  The readers copy page cache -> pinned memory (which the runtime places next to the device):
    from the other socket that copy crosses the inter-socket links and the read + host-to-device pipeline of a 2000-frame
    sequence took 14.5 instead of 10.5 ms (tools/r06_numa_probe.py at commit 1ab2c18)."""
    try:
        p = torch.cuda.get_device_properties(device)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return None
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        return cpus or None
    except (OSError, ValueError, AttributeError, RuntimeError):
        return None


def reader_pool(name, workers, cpus=None):
    """The process's pools of reader threads (thread start-up costs milliseconds here; the readers also keep their pinned
    staging buffers between calls).  `cpus`: the threads of a NEW pool are confined to these."""
    p = _pools.get(name)
    if p is None or p[1] < workers:
        from concurrent.futures import ThreadPoolExecutor

        def confine():
            if cpus:
                try:
                    os.sched_setaffinity(0, cpus)
                except OSError:
                    pass
        p = _pools[name] = (ThreadPoolExecutor(max_workers=max(1, workers), thread_name_prefix="gem-" + name, initializer=confine), workers)
    return p[0]


def drain(futures):
    """Cancel what has not started, wait for what has (its buffers are about to be reused or released)."""
    futures[:] = [f for f in futures if not f.done()]          # (the normal way out: everything has long finished)
    for f in futures:
        f.cancel()
    for f in futures:
        if not f.cancelled():
            try:
                f.result()
            except Exception:
                pass
    del futures[:]


def copy_stream(device):
    """The stream this reader thread copies on: the threads share N_COPY_STREAMS streams per device (handed out round-robin).
    Few, not one per thread: the runtime maps streams onto a handful of hardware queues, and a compute stream that lands in
    the same queue as a copying stream has its kernels held up behind that stream's copies (measured: a 7.6 ms optimiser call
    took 13.6 ms beside eight copying streams).  More than one, because copies of one stream run strictly one after the
    other with a gap between them."""
    with _copy_lock:
        st = _copy_streams.setdefault(device, [[], 0])
        if len(st[0]) < N_COPY_STREAMS:
            st[0].append(torch.cuda.Stream(device=device))
        st[1] += 1
        return st[0][(st[1] - 1) % len(st[0])]


def report_stream(device):
    """The device's stream for reading results back: on the compute stream a read-back would queue up behind whatever has been
    enqueued there since."""
    if device not in _report_streams:
        _report_streams[device] = torch.cuda.Stream(device=device)
    return _report_streams[device]


def thread_state(device):
    """The calling reader thread's state for `device`: `stream` (its copy stream), `stage` / `copied` (two pinned buffers and the
    event behind each one's last copy), `turn`, and `image`, a slot its user may keep a device buffer in."""
    tl = _reader_local
    if getattr(tl, "stream", None) is None or tl.device != device:
        tl.stream, tl.device = copy_stream(device), device
        tl.stage, tl.copied, tl.turn, tl.image = [None, None], [None, None], 0, None
    return tl


def staging_buffer(tl, nbytes):
    """One of this reader thread's two pinned staging buffers (uint8, at least nbytes), free to be written: the copy that last
    used it has left it.  Two alternate, so that the next file is read while the last one is still crossing PCIe.  Returns
    (k, buffer); the caller records the event behind its copy in `tl.copied[k]`."""
    k = tl.turn
    tl.turn ^= 1
    if tl.stage[k] is None or tl.stage[k].numel() < nbytes:
        tl.stage[k] = torch.empty(nbytes + (1 << 20), dtype=torch.uint8).pin_memory()
    if tl.copied[k] is not None:
        tl.copied[k].synchronize()
    return k, tl.stage[k]


class Scratch:
    """A pinned block for SMALL arrays (poses, cameras, window tables, payload offsets, report inputs): they go to the device
    with asynchronous copies from it.  (A pageable copy blocks the calling thread until the copy engines get to it -- behind
    the readers' 8 MB slices that is milliseconds per array.)"""

    def __init__(self, device):
        self.device, self.buf, self.at = device, None, 0

    def reset(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(2 * nbytes, dtype=torch.uint8).pin_memory()
        self.at = 0

    def upload(self, a, dtype):
        a = np.asarray(a)
        n = int(a.size) * torch.empty(0, dtype=dtype).element_size()
        if self.buf is None or self.at + n + 64 > self.buf.numel():          # (more than reset() was told: an ordinary copy)
            return torch.as_tensor(a, dtype=dtype).to(self.device).contiguous()
        view = self.buf[self.at:self.at + n].view(dtype).view(a.shape)
        self.at += (n + 63) // 64 * 64
        np.copyto(view.numpy(), a, casting="unsafe")
        return view.to(self.device, non_blocking=True)


# ------------------------------------------------------------------------------------------------------------------ device -> files
def kept_bytes(device, key, part, nbytes, host=False, grow_only=False):
    """The uint8 buffer of exactly `nbytes` kept between calls under (device, key, part): on the device, or (host=True) in host
    memory, pinned unless the device is the CPU.  Re-made whenever `nbytes` differs from what is kept -- with grow_only, only when
    it is more, and the buffer may then be larger than `nbytes`."""
    device = torch.device(device)
    buf = _kept.get((device, key, part))
    if buf is None or (buf.numel() < nbytes if grow_only else buf.numel() != nbytes):
        _kept.pop((device, key, part), None)          # (the old one goes before the new one is made)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cpu" if host else device)
        if host and device.type != "cpu":
            buf = buf.pin_memory()
        _kept[(device, key, part)] = buf
    return buf


def release_kept(key):
    """Give back every buffer kept under `key` (on all devices)."""
    for k in [k for k in _kept if k[1] == key]:
        del _kept[k]


def stream_out(device, key, nbytes, batches, produce, consume, side_bytes=0, waited=None):
    """`batches` batches of bytes made on the device, each at most `nbytes`, through two alternating pinned buffers to the caller's
    writer threads: while batch k is being written to its files, batch k+1 is made and crosses PCIe into the other buffer.

    `produce(k, device_buffer)` enqueues batch k's kernels on the current stream, writing into `device_buffer` (uint8 [nbytes]; the
    caller takes its 2-D views), and returns how many of its bytes are valid -- or (valid, side): `side` a small contiguous device
    tensor of `side_bytes` bytes that travels beside the batch.  `valid` may instead be a uint8 device tensor of the caller's own
    (a batch that outgrew `nbytes`): that one comes to the host with a blocking copy and is handed over in its turn, without overlap.
    `consume(k, host_bytes, side)` is called on this thread once batch k has arrived and batch k+1 has been enqueued: `host_bytes`
    is the uint8 host tensor of the valid bytes, `side` the uint8 host tensor [side_bytes] (None without; good until `consume`
    returns).  It submits the batch's file work to a pool of the caller's and returns the futures -- best as a generator: the loop
    takes them over one by one, so that those already submitted are looked after even if a later `submit` raises -- or STOP:
    nothing more is enqueued, the batch already under way is dropped, and the loop settles what it has.

    Batch k uses buffer k % 2; before `produce` may touch it, every future of the batch that last used it has been awaited (a
    writer's exception surfaces there), and both buffers are settled before this returns: every file is complete.  On any
    exception the last copy is waited for, futures that have not started are cancelled, the others awaited with their errors
    swallowed, and the exception goes on: nothing reads or writes the buffers once this has returned.  The buffers are kept
    between calls per (device, key) (`kept_bytes`, `release_kept`).  Everything runs on the current stream.  A `device` of type
    cpu takes ordinary host memory, synchronous copies and no event.  `waited(name, seconds)`: told the time spent waiting for a
    batch to arrive ("copy") and for a buffer's writers ("file")."""
    if batches < 1:
        return
    device = torch.device(device)
    on_gpu = device.type != "cpu"
    host = [kept_bytes(device, key, "host%d" % i, nbytes, host=True) for i in range(2)]
    sides = [kept_bytes(device, key, "side%d" % i, side_bytes, host=True) for i in range(2)] if side_bytes else None
    dev = kept_bytes(device, key, "device", nbytes)
    writing, arrived, last = [[], []], None, None          # per buffer: its batch's futures; the batch under way; the last copy's event

    def wait(name, fn):
        t0 = time.perf_counter()
        try:
            fn()
        finally:
            if waited is not None:
                waited(name, time.perf_counter() - t0)

    def settle(futures):
        for f in futures:
            wait("file", f.result)
        del futures[:]

    def hand_over(batch):
        k, ev, data, side = batch
        if ev is not None:
            wait("copy", ev.synchronize)
        out = consume(k, data, side)
        if out != STOP:
            for f in out:
                writing[k % 2].append(f)
        return out

    try:
        for k in range(batches):
            settle(writing[k % 2])
            out = produce(k, dev)
            valid, side = out if isinstance(out, tuple) else (out, None)
            if torch.is_tensor(valid):
                data = valid.cpu()
            else:
                data = host[k % 2][:valid]
                data.copy_(dev[:valid], non_blocking=True)
            if side is not None:
                sides[k % 2].copy_(side.view(torch.uint8).view(-1), non_blocking=True)
                side = sides[k % 2]
            if on_gpu:
                last = torch.cuda.Event()
                last.record(torch.cuda.current_stream())
            batch, arrived = arrived, (k, last, data, side)
            if batch is not None and hand_over(batch) == STOP:
                arrived = None
                break
        if arrived is not None:
            hand_over(arrived)
        settle(writing[0])
        settle(writing[1])
    finally:
        if last is not None:
            last.synchronize()          # (the stream's last copy: with it every earlier one has left the buffers alone)
        drain(writing[0])
        drain(writing[1])


def release():
    """Give back what this module keeps between calls: the copy and report streams, the outbound buffers and the reader threads
    (with their pinned staging buffers and device images).  Not to be called while a call that uses them is in flight."""
    _kept.clear()
    _copy_streams.clear()
    _report_streams.clear()
    pools = list(_pools.values())
    _pools.clear()
    for p, _ in pools:
        p.shutdown(wait=True)
