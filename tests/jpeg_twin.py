"""numpy twin of the device's JPEG encoder, written from DESIGN.md section 6j ("The format"), not from the kernel: `encode` /
`coefficients` / `header`, a baseline decoder for such files (`decode`: Huffman decode, dequantise, float64 IDCT, inverse colour,
crop) and `symbol_stats`, which says what a file's entropy data exercises.  The Annex K tables are typed in here a second time."""
import struct

import numpy as np

Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61,
          12, 12, 14, 19, 26, 58, 60, 55,
          14, 13, 16, 24, 40, 57, 69, 56,
          14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77,
          24, 35, 55, 64, 81, 104, 113, 92,
          49, 64, 78, 87, 103, 121, 120, 101,
          72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99,
            18, 21, 26, 66, 99, 99, 99, 99,
            24, 26, 56, 99, 99, 99, 99, 99,
            47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    list(bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HEADER_BYTES = 629


def zigzag():
    """zigzag index -> natural index y * 8 + x: diagonals d = x + y ascending, odd d with y ascending, even d with x ascending."""
    order = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]
        if d % 2 == 0:
            cells.sort(key=lambda c: c[1])
        order += [y * 8 + x for y, x in cells]
    return order


ZIGZAG = zigzag()


def quant_tables(quality):
    """[2][64] in natural order: the Annex K tables under the IJG quality rule."""
    if not 1 <= quality <= 100:
        raise ValueError("quality is 1 .. 100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (Q_LUMA, Q_CHROMA)]


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return np.rint(2.0 ** 14 * (c / 2.0) * np.cos((2 * x + 1) * u * np.pi / 16.0)).astype(np.int64)


def canonical(bits, vals):
    """symbol -> (code, length)"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


DC_CODES = [canonical(DC_BITS[i], DC_VALS[i]) for i in range(2)]
AC_CODES = [canonical(AC_BITS[i], AC_VALS[i]) for i in range(2)]


def image_of(scan, W, H):
    """[H,W,3] from a scanline stream of H rows of 1 + 3 W bytes (the filter byte is ignored)."""
    rows = np.frombuffer(bytes(scan), dtype=np.uint8)[:H * (1 + 3 * W)].reshape(H, 1 + 3 * W)
    return rows[:, 1:].reshape(H, W, 3).copy()


def coefficients(img, quality=90):
    """int16 [3, Hp/8, Wp/8, 64]: the quantised coefficients of Y, Cb, Cr in zigzag order."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    img = np.pad(img, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = img[..., 0], img[..., 1], img[..., 2]
    planes = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
              (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32768) >> 16,
              (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32768) >> 16]
    p = np.stack([np.clip(q, 0, 255) - 128 for q in planes]).reshape(3, Hp // 8, 8, Wp // 8, 8)
    C = dct_matrix()
    F = np.einsum("vy,cbyax,ux->cbavu", C, p, C)          # exact in int64
    qt = np.array(quant_tables(quality), dtype=np.int64)
    D = np.stack([qt[0], qt[1], qt[1]]).reshape(3, 1, 1, 8, 8) << 28
    level = np.sign(F) * ((np.abs(F) + D // 2) // D)
    return level.reshape(3, Hp // 8, Wp // 8, 64)[..., ZIGZAG].astype(np.int16)


def header(W, H, quality):
    qt = quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i in range(2):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(qt[i][n] for n in ZIGZAG)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for i in range(2):
        for ac, (bits, vals) in enumerate(((DC_BITS[i], DC_VALS[i]), (AC_BITS[i], AC_VALS[i]))):
            out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (ac << 4) | i) + bytes(bits) + bytes(vals)
    out += b"\xff\xdd" + struct.pack(">HH", 4, (W + 7) // 8)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])
    assert len(out) == HEADER_BYTES
    return out


def _magnitude(v):
    s = int(abs(v)).bit_length()
    return s, (v if v > 0 else v + (1 << s) - 1)


def _segment(coef_row):
    """One MCU row [3, nbx, 64] -> its entropy data: padded with 1-bits, then stuffed."""
    acc, n = 0, 0
    pred = [0, 0, 0]
    for bx in range(coef_row.shape[1]):
        for c in range(3):
            blk = [int(v) for v in coef_row[c, bx]]
            t = 0 if c == 0 else 1
            s, mag = _magnitude(blk[0] - pred[c])
            pred[c] = blk[0]
            code, length = DC_CODES[t][s]
            acc, n = (((acc << length) | code) << s) | mag, n + length + s
            last = max([k for k in range(1, 64) if blk[k]], default=0)
            run = 0
            for k in range(1, last + 1):
                if blk[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    code, length = AC_CODES[t][0xF0]
                    acc, n = (acc << length) | code, n + length
                    run -= 16
                s, mag = _magnitude(blk[k])
                code, length = AC_CODES[t][(run << 4) | s]
                acc, n = (((acc << length) | code) << s) | mag, n + length + s
                run = 0
            if last < 63:
                code, length = AC_CODES[t][0]
                acc, n = (acc << length) | code, n + length
    pad = -n % 8
    acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
    return acc.to_bytes(n // 8, "big").replace(b"\xff", b"\xff\x00")


def encode(img, quality=90, coef=None):
    """A complete JPEG file of img [H,W,3] uint8."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    coef = coefficients(img, quality) if coef is None else coef
    out = [header(W, H, quality)]
    for by in range(coef.shape[1]):
        if by:
            out.append(bytes([0xFF, 0xD0 + (by - 1) % 8]))
        out.append(_segment(coef[:, by]))
    return b"".join(out) + b"\xff\xd9"


def avi_chunk(jpeg):
    return b"00dc" + struct.pack("<I", len(jpeg)) + jpeg + (b"\0" if len(jpeg) % 2 else b"")


# ------------------------------------------------------------------------------------------------------------------ reading
class _Bits:
    def __init__(self, data):
        self.v, self.n = int.from_bytes(data, "big"), 8 * len(data)

    def take(self, k):
        if k > self.n:
            raise ValueError("the entropy data ends inside a symbol")
        self.n -= k
        return (self.v >> self.n) & ((1 << k) - 1)

    def symbol(self, lookup):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (code, length) in lookup:
                return lookup[(code, length)]
        raise ValueError("no such Huffman code")


def _parse(data):
    """The segments of a baseline file of this kind -> dict; ValueError for anything else."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    at, info = 2, {"qt": {}, "dc": {}, "ac": {}, "dri": 0}
    while True:
        if data[at] != 0xFF:
            raise ValueError("no marker at %d" % at)
        kind, n = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        body = data[at + 4:at + 2 + n]
        at += 2 + n
        if kind == 0xDB:
            info["qt"][body[0]] = list(body[1:65])
        elif kind == 0xC0:
            prec, H, W, nc = struct.unpack(">BHHB", body[:6])
            comps = [tuple(body[6 + 3 * i:9 + 3 * i]) for i in range(nc)]
            if prec != 8 or nc != 3 or any(c[1] != 0x11 for c in comps):
                raise ValueError("not 8-bit, three components, 4:4:4")
            info.update(H=H, W=W, tq=[c[2] for c in comps])
        elif kind == 0xC4:
            bits, vals = list(body[1:17]), list(body[17:])
            info["ac" if body[0] >> 4 else "dc"][body[0] & 15] = {(c, l): s for s, (c, l) in canonical(bits, vals).items()}
        elif kind == 0xDD:
            info["dri"] = struct.unpack(">H", body)[0]
        elif kind == 0xDA:
            info["tables"] = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(3)]
            break
        elif kind != 0xE0:
            raise ValueError("unexpected marker %02X" % kind)
    if data[-2:] != b"\xff\xd9":
        raise ValueError("no EOI at the end")
    info["entropy"] = data[at:-2]
    return info


def _walk(data):
    """-> (info, coefficients [3, nby, nbx, 64] in zigzag order, stats)"""
    info = _parse(bytes(data))
    nbx, nby = (info["W"] + 7) // 8, (info["H"] + 7) // 8
    if info["dri"] != nbx:
        raise ValueError("DRI is not one MCU row")
    ent, segs, markers, start, i = info["entropy"], [], [], 0, 0
    while i < len(ent) - 1:
        if ent[i] == 0xFF and ent[i + 1] != 0:
            if not 0xD0 <= ent[i + 1] <= 0xD7:
                raise ValueError("marker %02X inside the entropy data" % ent[i + 1])
            segs.append(ent[start:i])
            markers.append(ent[i + 1])
            start = i + 2
            i += 2
        else:
            i += 2 if ent[i] == 0xFF else 1
    segs.append(ent[start:])
    if len(segs) != nby or markers != [0xD0 + k % 8 for k in range(nby - 1)]:
        raise ValueError("%d segments for %d MCU rows, markers %s" % (len(segs), nby, markers))
    stats = {"zrl": 0, "stuffed": sum(s.count(b"\xff\x00") for s in segs), "dc_category": 0, "ac_category": 0, "markers": markers}
    coef = np.zeros((3, nby, nbx, 64), dtype=np.int16)
    for by, seg in enumerate(segs):
        bits, pred = _Bits(seg.replace(b"\xff\x00", b"\xff")), [0, 0, 0]
        for bx in range(nbx):
            for c in range(3):
                tdc, tac = info["tables"][c]
                s = bits.symbol(info["dc"][tdc])
                stats["dc_category"] = max(stats["dc_category"], s)
                v = bits.take(s)
                pred[c] += v if s == 0 or v >> (s - 1) else v - (1 << s) + 1
                coef[c, by, bx, 0] = pred[c]
                k = 1
                while k < 64:
                    sym = bits.symbol(info["ac"][tac])
                    run, s = sym >> 4, sym & 15
                    if s == 0:
                        if run != 15:
                            if run:
                                raise ValueError("an AC symbol %02X" % sym)
                            break
                        stats["zrl"] += 1
                        k += 16
                        continue
                    k += run
                    if k > 63:
                        raise ValueError("a run leaves the block")
                    stats["ac_category"] = max(stats["ac_category"], s)
                    v = bits.take(s)
                    coef[c, by, bx, k] = v if v >> (s - 1) else v - (1 << s) + 1
                    k += 1
        left = bits.n
        if left >= 8 or bits.take(left) != (1 << left) - 1:
            raise ValueError("segment %d does not end padded with 1-bits" % by)
    return info, coef, stats


def symbol_stats(data):
    """{"zrl": ZRL symbols, "stuffed": stuffed bytes, "dc_category", "ac_category": the largest, "markers": the RST markers seen}"""
    return _walk(data)[2]


def decode(data):
    """A file of this kind -> uint8 [H,W,3]."""
    info, coef, _ = _walk(data)
    nby, nbx = coef.shape[1:3]
    nat = np.zeros(coef.shape, dtype=np.float64)
    nat[..., ZIGZAG] = coef
    q = np.array([info["qt"][t] for t in info["tq"]], dtype=np.float64)          # zigzag order in the file
    qn = np.zeros((3, 64))
    qn[:, ZIGZAG] = q
    F = (nat * qn[:, None, None, :]).reshape(3, nby, nbx, 8, 8)
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    A = np.where(u == 0, np.sqrt(0.5), 1.0) / 2.0 * np.cos((2 * x + 1) * u * np.pi / 16.0)          # [u][x]
    p = np.einsum("vy,cbavu,ux->cbyax", A, F, A).reshape(3, nby * 8, nbx * 8) + 128.0
    Y, Cb, Cr = p[0], p[1] - 128.0, p[2] - 128.0
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:info["H"], :info["W"]]
