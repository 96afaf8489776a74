"""How bytes get from the host to the device: reader threads next to the device, two copy streams, pinned staging buffers.

Nothing here knows about chunks, windows or MAT files.  `whole_sequence` (chunk pickles) and `prepare` (the pose network's
.mat files) are built on it:

  * `reader_pool`: the process's named pools of reader threads, optionally confined to the CPUs `cpus_near` the device;
  * `copy_stream` / `report_stream`: the few streams the copies and the read-backs run on;
  * `thread_state` / `staging_buffer`: a reader thread's two alternating pinned buffers and the events that guard them;
  * `Scratch`: a pinned block from which small arrays go up asynchronously;
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


def release():
    """Give back what this module keeps between calls: the copy and report streams and the reader threads (with their pinned
    staging buffers and device images).  Not to be called while a call that uses them is in flight."""
    _copy_streams.clear()
    _report_streams.clear()
    pools = list(_pools.values())
    _pools.clear()
    for p, _ in pools:
        p.shutdown(wait=True)
