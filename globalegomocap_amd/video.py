"""Rendered frames as one clip that plays: Motion-JPEG in an AVI file, encoded on the device.

`write_video` takes the images the renderers draw (`render._write_scanlines`' `draw(lo, n, out)` contract), turns every batch into
baseline JPEG images on the device (`WindowEngine.jpeg_encode_into`: gem_jpeg_encode, already framed as the file's `00dc` chunks) and
moves only those bytes -- a few tens of KB per frame instead of the scanlines -- through `staging.stream_out` to one writer
thread, which appends them to the file and keeps the index.  The container is RIFF AVI 1.0 (no OpenDML: a file ends below 2 GiB),
one video stream `MJPG`, an `idx1` index; `read_avi` reads such a file back, strictly.  No player exists where this was written: the
container is checked against its specification and by reading it back (6j, "Container").
"""
import os
import struct

PINNED_BYTES = 32 << 20          # each of the two pinned buffers the chunks cross PCIe through, and the device buffer they are made in
SCAN_BYTES = 64 << 20            # the device buffer the scanlines are drawn into (`render.PINNED_BYTES`: the same batches)
DEFAULT_FPS, DEFAULT_QUALITY = 25, 90          # of a clip wherever a caller gives none (`report.Outputs` resolves None to them)
MAX_FILE = (1 << 31) - 1
HEADER_BYTES = 224               # everything in front of the first chunk; the 'movi' fourcc is at 220
AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10


def _check(width, height, fps, quality):
    if not (1 <= int(width) <= 1024 and 1 <= int(height) <= 16384):
        raise ValueError("a clip is 1 .. 1024 pixels wide and 1 .. 16384 high, got %d x %d" % (width, height))
    if not fps > 0:
        raise ValueError("video_fps must be positive, got %r" % (fps,))
    if not (int(quality) == quality and 1 <= quality <= 100):
        raise ValueError("video_quality is a whole number 1 .. 100, got %r" % (quality,))


def check_options(fps, quality):
    """ValueError for a frame rate or a JPEG quality no clip can be written with."""
    _check(1, 1, fps, quality)


def _header(width, height, fps, frames, largest, movi_bytes):
    """The 224 bytes in front of the first chunk; `movi_bytes` = the bytes of all chunks."""
    avih = struct.pack("<14I", int(round(1e6 / fps)), 0, 0, AVIF_HASINDEX, frames, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, 1000, int(round(1000 * fps)), 0, frames, largest, 0xFFFFFFFF, 0,
                       0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", 3 * width * height, 0, 0, 0, 0)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    riff_bytes = 4 + 8 + len(hdrl) + 8 + 4 + movi_bytes + 8 + 16 * frames
    out = b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + \
        b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
    assert len(avih) == 56 and len(strh) == 56 and len(strf) == 40 and len(out) == HEADER_BYTES
    return out


class AviWriter:
    """One AVI file being written: `append` takes a run of complete `00dc` chunks, `close` writes the index and patches the counts
    and sizes into the header.  A run that would take the file past 2^31 - 1 bytes closes it as a valid file of the frames written
    so far and raises OverflowError."""

    def __init__(self, path, width, height, fps=DEFAULT_FPS, quality=DEFAULT_QUALITY):
        _check(width, height, fps, quality)
        self.path, self.width, self.height, self.fps = path, int(width), int(height), float(fps)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.file = open(path, "wb")
        self.file.write(_header(self.width, self.height, self.fps, 0, 0, 0))
        self.index, self.movi_bytes, self.largest = [], 0, 0

    def append(self, run, offsets):
        """`run`: bytes-like, chunk i at offsets[i] .. offsets[i+1] (offsets[0] = 0): '00dc', the frame's length, the frame, a zero
        byte behind an odd length."""
        run = memoryview(run).cast("B")
        n, total = len(offsets) - 1, offsets[-1]
        if offsets[0] != 0 or total > len(run):
            raise ValueError("the chunks' offsets do not fit the run of %d bytes" % len(run))
        if HEADER_BYTES + self.movi_bytes + total + 8 + 16 * (len(self.index) + n) > MAX_FILE:
            frames = len(self.index)
            self.close()
            raise OverflowError("%s: the next %d frames would take the file past 2^31 - 1 bytes; it holds the %d frames before them"
                                % (self.path, n, frames))
        entries = []
        for i in range(n):
            lo, hi = offsets[i], offsets[i + 1]
            size = struct.unpack("<I", run[lo + 4:lo + 8])[0] if hi - lo >= 8 else -1
            if bytes(run[lo:lo + 4]) != b"00dc" or hi - lo != 8 + size + (size & 1):
                raise ValueError("chunk %d of the run is not a '00dc' chunk of its length" % i)
            entries.append((4 + self.movi_bytes + lo, size))
        self.file.write(run[:total])
        self.index += entries
        self.movi_bytes += total
        self.largest = max([self.largest] + [s for _, s in entries])

    def append_frames(self, frames):
        """JPEG files (bytes) as chunks."""
        chunks = [b"00dc" + struct.pack("<I", len(f)) + bytes(f) + (b"\0" if len(f) & 1 else b"") for f in frames]
        at = [0]
        for c in chunks:
            at.append(at[-1] + len(c))
        self.append(b"".join(chunks), at)

    def close(self):
        if self.file is None:
            return
        f, self.file = self.file, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)) +
                    b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, at, size) for at, size in self.index))
            f.seek(0)
            f.write(_header(self.width, self.height, self.fps, len(self.index), self.largest, self.movi_bytes))
        finally:
            f.close()


def write_avi(path, frames, width, height, fps=DEFAULT_FPS):
    """JPEG files (a list of bytes) -> one AVI file; host only.  Returns the number of frames."""
    w = AviWriter(path, width, height, fps)
    try:
        w.append_frames(frames)
    finally:
        w.close()
    return len(frames)


def read_avi(path):
    """An AVI file of this module's making -> (fps, width, height, [frame bytes]).  Strict: the RIFF and LIST sizes must be the
    file's, the headers the ones `AviWriter` writes for the frames found, the index present and in agreement with `movi`, nothing
    behind it.  ValueError otherwise."""
    with open(path, "rb") as f:
        data = f.read()

    def fail(what):
        raise ValueError("%s: %s" % (path, what))

    def u32(at):
        if at + 4 > len(data):
            fail("truncated at byte %d" % at)
        return struct.unpack("<I", data[at:at + 4])[0]
    if len(data) < HEADER_BYTES or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        fail("no RIFF AVI header")
    if u32(4) != len(data) - 8:
        fail("the RIFF size says %d bytes, the file has %d" % (u32(4) + 8, len(data)))
    if data[12:16] != b"LIST" or data[20:24] != b"hdrl" or u32(16) != 192 or data[24:28] != b"avih" or u32(28) != 56:
        fail("no hdrl list with an avih of 56 bytes")
    avih = struct.unpack("<14I", data[32:88])
    if data[88:92] != b"LIST" or u32(92) != 116 or data[96:104] != b"strlstrh" or u32(104) != 56:
        fail("no strl list with a strh of 56 bytes")
    strh = struct.unpack("<4s4sIHHIIIIIIII4h", data[108:164])
    if data[164:168] != b"strf" or u32(168) != 40:
        fail("no strf of 40 bytes")
    strf = struct.unpack("<IiiHH4sIiiII", data[172:212])
    if data[212:216] != b"LIST" or data[220:224] != b"movi":
        fail("no movi list behind the headers")
    movi_end = 220 + u32(216)
    if movi_end > len(data):
        fail("the movi list leaves the file")
    frames, found, at = [], [], 224
    while at < movi_end:
        if at + 8 > movi_end or data[at:at + 4] != b"00dc":
            fail("no '00dc' chunk at byte %d" % at)
        size = u32(at + 4)
        end = at + 8 + size + (size & 1)
        if end > movi_end:
            fail("the chunk at byte %d leaves the movi list" % at)
        if size & 1 and data[end - 1] != 0:
            fail("the pad byte of the chunk at byte %d is not zero" % at)
        frames.append(data[at + 8:at + 8 + size])
        found.append((at - 220, size))
        at = end
    if data[movi_end:movi_end + 4] != b"idx1":
        fail("no idx1 behind the movi list")
    if u32(movi_end + 4) != 16 * len(frames) or movi_end + 8 + 16 * len(frames) != len(data):
        fail("the index does not hold 16 bytes for each of the %d frames, or something follows it" % len(frames))
    for i, (where, size) in enumerate(found):
        e = movi_end + 8 + 16 * i
        if data[e:e + 4] != b"00dc" or struct.unpack("<III", data[e + 4:e + 16]) != (AVIIF_KEYFRAME, where, size):
            fail("index entry %d disagrees with the movi list" % i)
    width, height, n = avih[8], avih[9], len(frames)
    largest = max([0] + [s for _, s in found])
    if strh[7] == 0 or strh[6] != 1000:
        fail("dwScale / dwRate are not 1000 / (1000 fps)")
    fps = strh[7] / 1000.0
    expected = _header(width, height, fps, n, largest, movi_end - 224)          # (dwMicroSecPerFrame: rounded from the fps given, not from dwRate)
    if data[:32] + data[36:HEADER_BYTES] != expected[:32] + expected[36:] or abs(avih[0] - 1e6 / fps) > 1.0:
        fail("the headers are not the ones of %d frames of %d x %d (largest %d bytes)" % (n, width, height, largest))
    if (strf[1], strf[2]) != (width, height) or strh[:2] != (b"vids", b"MJPG"):
        fail("the stream format disagrees with the main header")
    return fps, width, height, frames


def write_video(engine, draw, W, H, n_frames, path, fps=DEFAULT_FPS, quality=DEFAULT_QUALITY, timings=None):
    """`n_frames` images of W x H pixels as one Motion-JPEG clip `path`; `draw(lo, n, out)` renders the images lo .. lo + n into the
    rows of `out`, a uint8 device tensor [n, stride] (`render._write_scanlines`' contract).  Batches as there: the scanlines are
    drawn into a device buffer, encoded on the device as the file's chunks (`WindowEngine.jpeg_encode_into`), the chunk offsets read
    back, and only offsets[n] bytes cross PCIe (`staging.stream_out`); one writer thread appends them and keeps the index
    (`AviWriter`).  A batch whose chunks outgrow the loop's buffer -- noise at quality 100 -- is encoded again into a buffer of its own
    and written without the overlap.  Runs on the current stream; the file is complete and closed on return; returns
    n_frames.  timings: a dict that receives the seconds spent waiting in the phases render, encode, copy and file."""
    import time
    import torch
    from . import render
    from .staging import kept_bytes, reader_pool, stream_out
    _check(W, H, fps, quality)
    n_frames = int(n_frames)
    if n_frames < 0:
        raise ValueError("n_frames < 0")
    lay = render.layout(W, H)
    per = max(1, min(SCAN_BYTES // lay.stride, n_frames))
    writer = AviWriter(path, W, H, fps, quality)
    pool = reader_pool("video", 1)          # one writer: the runs are appended in order
    laps = {"render": 0.0, "encode": 0.0, "copy": 0.0, "file": 0.0}
    offsets_of = {}          # batch -> its chunks' offsets, from `produce` to `consume`

    def lap(name, t0, sync=False):
        if timings is not None and sync:
            torch.cuda.current_stream().synchronize()
        laps[name] += time.perf_counter() - t0
        return time.perf_counter()

    def waited(name, seconds):
        laps[name] += seconds

    def produce(k, out):
        n = min(per, n_frames - k * per)
        scan = scanlines[:n]
        t0 = time.perf_counter()
        draw(k * per, n, scan)
        t0 = lap("render", t0, True)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=engine.device)
        engine.jpeg_encode_into(scan, W, H, quality, True, out, offsets)
        at = offsets_of[k] = offsets.tolist()          # the one read-back of the batch
        lap("encode", t0)
        if at[n] <= out.numel():
            return at[n]
        big = torch.empty(at[n], dtype=torch.uint8, device=engine.device)
        engine.jpeg_encode_into(scan, W, H, quality, True, big, offsets)
        return big

    def consume(k, data, side):
        return [pool.submit(writer.append, data.numpy(), offsets_of.pop(k))]

    try:
        if n_frames:          # the device buffer the scanlines are drawn into
            scanlines = kept_bytes(engine.device, "video", "scanlines", per * lay.stride, grow_only=True)[:per * lay.stride].view(per, lay.stride)
        stream_out(engine.device, "video", PINNED_BYTES, (n_frames + per - 1) // per, produce, consume, waited=waited)
    finally:
        t0 = time.perf_counter()
        writer.close()
        lap("file", t0)
    if timings is not None:
        timings.update(laps)
    return n_frames


def release():
    """Give back the pinned and device buffers `write_video` keeps between calls."""
    from .staging import release_kept
    release_kept("video")
