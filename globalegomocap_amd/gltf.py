"""Results as one glTF 2.0 binary file (`.glb`): skinned, animated skeletons that Blender, Unity, Unreal, three.js and any browser viewer
open and play.

One file holds several sequences of equal length -- the estimated, the optimised and, where there is one, the ground-truth skeleton --
each as a skinned mesh (the spheres and cylinders of `--save`) in a colour of its own on the BVH route's 19-node skeleton, all driven by
ONE animation, so that they play in sync.  The library makes the per-sequence parts on the device: the rest lengths (gem_bvh_rest), the
rest-pose mesh with its skinning (gem_gltf_rest_mesh) and the animation block -- key times, the Hips' translation, 15 local rotations as
unit quaternions whose sign is continuous from key to key (gem_gltf_animation).  Python writes the JSON chunk, the shared index buffer
and the inverse bind matrices; `write_gltf` moves the BIN chunk device -> pinned memory -> file in slices through two alternating pinned
buffers.  `read_glb` and `joint_positions` read such a file back into joint positions.

    python -m globalegomocap_amd.gltf out/<dataset>/<chunk>/result_pose.pkl --out FILE.glb [--fps F] [--align true] [--upright] [--foot_lock]
"""
import ctypes as C
import json
import os
import struct
from collections import namedtuple

import numpy as np

from . import _capi
from . import bvh
from ._binding import _ptr, _stream, check_tensor
from .bvh import DEFAULT_FPS, NODE_NAMES, new_counter
from .meshes import _alignment, _sequence, _upright, result_poses

Layout = namedtuple("Layout", "nodes rotating vertices triangles vertex_stride vertex_bytes rotating_nodes offsets block_bytes frame_bytes")
Section = namedtuple("Section", "name offset nbytes data")          # data: the host's bytes, or None for what the device makes
Parsed = namedtuple("Parsed", "json accessors bin")
PINNED_BYTES = 16 << 20          # each of the two pinned buffers the BIN chunk crosses PCIe through, whatever the file's size
FILE_NAME = "result.glb"
SEQUENCE_NAMES = ("estimated", "optimized", "gt")          # the keys of `render.PALETTE`
MAGIC, VERSION, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 2, 0x4E4F534A, 0x004E4942
FLOAT, UBYTE, USHORT, ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 5126, 5121, 5123, 34962, 34963
_COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
_DTYPES = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}

_indices = None


def layout(n_frames):
    """The counts of the file's skeleton and mesh and the byte offsets of the 17 arrays of an animation block of `n_frames` frames
    (gem_gltf_layout); needs no GPU."""
    lib = _capi.load_library()
    out = (C.c_int64 * _capi.GLTF_LAYOUT)()
    _capi.check(lib.gem_gltf_layout(int(n_frames), out), lib)
    v = [int(x) for x in out]
    return Layout(*v[:6], tuple(v[6:21]), tuple(v[21:38]), v[38], v[39])


def animation(engine, seq_d, crt, fps, bad=None, out=None):
    """The animation block of `seq_d` [F,15,3] (contiguous float64 device tensor) behind `crt` ([13] from `engine.sequence_align`, or
    None) at `fps` keys per second (gem_gltf_animation) -> (uint8 device tensor [layout(F).block_bytes], `out` when given (16-byte
    aligned); the counter).  bad: a `bvh.new_counter` that every frame with a number that is not finite raises; a new one when None.
    No synchronisation; the same bytes on every call."""
    import torch
    F = seq_d.shape[0]
    n = layout(F).block_bytes
    if out is None:
        out = torch.zeros(n, device=seq_d.device, dtype=torch.uint8)          # (zeros: the padding between the arrays is file content)
    check_tensor(out, torch.uint8, at_least=n, error=ValueError("animation: out must be a contiguous uint8 device tensor of at least %d bytes" % n))
    if bad is None:
        bad = new_counter(seq_d.device)
    _capi.check(engine.lib.gem_gltf_animation(_ptr(seq_d), F, _ptr(crt), C.c_double(float(fps)), _ptr(out), _ptr(bad), _stream()), engine.lib)
    return out[:n], bad


def rest_mesh(engine, rest, out=None):
    """The rest-pose mesh of the skeleton with the rest lengths `rest` ([19] f64 device tensor, `bvh.rest_lengths`) with its skinning
    (gem_gltf_rest_mesh) -> (uint8 device tensor [414 720]: 12 960 vertices of 32 bytes, `out` when given; its bounds, f32 [6]: the
    minimum and the maximum of the positions).  No synchronisation."""
    import torch
    n = layout(0).vertex_bytes
    if out is None:
        out = torch.empty(n, device=rest.device, dtype=torch.uint8)
    check_tensor(out, torch.uint8, at_least=n, error=ValueError("rest_mesh: out must be a contiguous uint8 device tensor of at least %d bytes" % n))
    bounds = torch.empty(6, device=rest.device, dtype=torch.float32)
    _capi.check(engine.lib.gem_gltf_rest_mesh(_ptr(rest), _ptr(out), _ptr(bounds), _stream()), engine.lib)
    return out[:n], bounds


# ------------------------------------------------------------------------------------------------------------------ the document
def index_bytes():
    """The file's ONE index buffer, shared by all its skeletons: the 25 800 triangles of `meshes.constant`'s face block as uint16."""
    global _indices
    if _indices is None:
        from .meshes import constant, layout as mesh_layout
        faces = np.frombuffer(constant()[1], dtype=np.dtype([("n", "u1"), ("i", "<u4", 3)]), count=mesh_layout().triangles)
        if faces["i"].max() >= 1 << 16:
            raise ValueError("the mesh has more vertices than uint16 indices can name")
        _indices = faces["i"].astype("<u2").tobytes()
    return _indices


def rest_positions(rest):
    """Where the 19 nodes stand in the rest pose of the skeleton with the rest lengths `rest` [19]: Hips at the origin -> [19,3]."""
    tab, rest = bvh.tables(), np.asarray(rest, dtype=np.float64)
    pos = np.zeros((len(NODE_NAMES), 3))
    for n in range(1, len(NODE_NAMES)):
        pos[n] = pos[tab.parents[n]] + tab.rest_dirs[n] * rest[n]
    return pos


def section_table(names, n_frames):
    """The BIN chunk's sections for skeletons called `names` and `n_frames` keys, in file order, every offset a multiple of 16:
    `indices`, then per skeleton `<name>/inverse_bind`, `<name>/vertices` and `<name>/animation` -> ([Section], the chunk's length)."""
    lay = layout(n_frames)
    out, at = [], 0
    for name, n in [("indices", 6 * lay.triangles)] + [("%s/%s" % (s, part), n) for s in names
                                                          for part, n in (("inverse_bind", 64 * lay.nodes), ("vertices", lay.vertex_bytes),
                                                                          ("animation", lay.block_bytes))]:
        out.append(Section(name, at, n, None))
        at += (n + 15) // 16 * 16
    return out, at


def _linear(c):
    c = c / 255.0          # sRGB, as the PNG frames show it -> the linear value a glTF material holds
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def build_document(skeletons, n_frames, fps):
    """The file's JSON for `skeletons` = [(name, rest lengths [19], bounds [6], (r, g, b) of 255)] and `n_frames` keys at `fps` per
    second, and the BIN chunk's section table (`section_table`, with the host's sections -- the indices, the inverse bind matrices --
    filled in; the vertices and the animation block of every skeleton come from the device) -> (dict, [Section], the chunk's length).
    Pure host, needs no GPU.  Per skeleton: 19 joint nodes `<name>/<NODE_NAMES[i]>` whose translations are the rest offsets, a skin
    with the inverse bind matrices (translations: the rest pose has no rotation), a mesh node at the scene's root, a material.  One
    index buffer and ONE animation for all: `translation` on every Hips, `rotation` on every rotating node, LINEAR, on one shared
    array of key times."""
    if n_frames < 1:
        raise ValueError("a glTF animation needs at least one frame")
    if not (fps > 0 and np.isfinite(fps)):
        raise ValueError("fps must be positive, got %r" % (fps,))
    names = [s[0] for s in skeletons]
    if len(set(names)) != len(names) or not names:
        raise ValueError("the skeletons of a file need names of their own, got %r" % (names,))
    lay, tab = layout(n_frames), bvh.tables()
    N = lay.nodes
    sections, total = section_table(names, n_frames)
    where = {s.name: i for i, s in enumerate(sections)}
    views, accessors, nodes, meshes, skins, materials, samplers, channels, roots = [], [], [], [], [], [], [], [], []

    def view(offset, nbytes, **extra):
        views.append(dict(buffer=0, byteOffset=int(offset), byteLength=int(nbytes), **extra))
        return len(views) - 1

    def accessor(v, ctype, count, kind, offset=0, **extra):
        accessors.append(dict(bufferView=v, byteOffset=int(offset), componentType=ctype, count=int(count), type=kind, **extra))
        return len(accessors) - 1

    sections[0] = sections[0]._replace(data=index_bytes())
    indices = accessor(view(sections[0].offset, sections[0].nbytes, target=ELEMENT_ARRAY_BUFFER), USHORT, 3 * lay.triangles, "SCALAR")
    times = None
    kids = [[c for c in range(N) if tab.parents[c] == n] for n in range(N)]
    for si, (name, rest, bounds, rgb) in enumerate(skeletons):
        base = len(nodes)
        pos = rest_positions(rest)
        offsets = tab.rest_dirs * np.asarray(rest, dtype=np.float64)[:, None] + 0.0
        bounds = [float(np.float32(b)) for b in bounds]
        if not (np.isfinite(pos).all() and np.isfinite(bounds).all()):
            raise ValueError("the skeleton %s has rest lengths or bounds that are no numbers" % name)
        for n in range(N):
            node = dict(name="%s/%s" % (name, NODE_NAMES[n]), translation=[float(x) for x in offsets[n]])
            if kids[n]:
                node["children"] = [base + c for c in kids[n]]
            nodes.append(node)
        ib = where["%s/inverse_bind" % name]
        mats = np.tile(np.eye(4, dtype="<f4"), (N, 1, 1))
        mats[:, 3, :3] = -pos          # (column-major: a matrix's translation is its last column, elements 12 .. 14)
        sections[ib] = sections[ib]._replace(data=mats.tobytes())
        inverse_bind = accessor(view(sections[ib].offset, sections[ib].nbytes), FLOAT, N, "MAT4")
        vs = sections[where["%s/vertices" % name]]
        vv = view(vs.offset, vs.nbytes, byteStride=lay.vertex_stride, target=ARRAY_BUFFER)
        attributes = dict(POSITION=accessor(vv, FLOAT, lay.vertices, "VEC3", 0, min=bounds[:3], max=bounds[3:]),
                          NORMAL=accessor(vv, FLOAT, lay.vertices, "VEC3", 12),
                          JOINTS_0=accessor(vv, UBYTE, lay.vertices, "VEC4", 24),
                          WEIGHTS_0=accessor(vv, UBYTE, lay.vertices, "VEC4", 28, normalized=True))
        materials.append(dict(name=name, pbrMetallicRoughness=dict(baseColorFactor=[_linear(c) for c in rgb] + [1.0], metallicFactor=0.0,
                                                                   roughnessFactor=0.8)))
        meshes.append(dict(name=name, primitives=[dict(attributes=attributes, indices=indices, material=si, mode=4)]))
        skins.append(dict(name=name, joints=list(range(base, base + N)), skeleton=base, inverseBindMatrices=inverse_bind))
        nodes.append(dict(name=name, mesh=si, skin=si))
        roots.extend([base, base + N])
        an = sections[where["%s/animation" % name]]
        if times is None:          # the key times of the first block serve every sampler
            last = float(np.float32(float(n_frames - 1) / float(fps)))
            times = accessor(view(an.offset + lay.offsets[0], 4 * n_frames), FLOAT, n_frames, "SCALAR", min=[0.0], max=[last])
        out = accessor(view(an.offset + lay.offsets[1], 12 * n_frames), FLOAT, n_frames, "VEC3")
        samplers.append(dict(input=times, output=out, interpolation="LINEAR"))
        channels.append(dict(sampler=len(samplers) - 1, target=dict(node=base, path="translation")))
        for k, n in enumerate(lay.rotating_nodes):
            out = accessor(view(an.offset + lay.offsets[2 + k], 16 * n_frames), FLOAT, n_frames, "VEC4")
            samplers.append(dict(input=times, output=out, interpolation="LINEAR"))
            channels.append(dict(sampler=len(samplers) - 1, target=dict(node=base + n, path="rotation")))
    doc = dict(asset=dict(version="2.0", generator="globalegomocap_amd.gltf"), scene=0, scenes=[dict(name="result", nodes=roots)], nodes=nodes,
               meshes=meshes, skins=skins, materials=materials, animations=[dict(name="result", samplers=samplers, channels=channels)],
               accessors=accessors, bufferViews=views, buffers=[dict(byteLength=int(total))])
    return doc, sections, total


def container_head(doc, bin_bytes):
    """What stands in front of the BIN chunk's bytes: the 12-byte header, the JSON chunk (padded with spaces to a multiple of 4) and the
    BIN chunk's 8-byte header, for a BIN chunk of `bin_bytes` bytes (a multiple of 4)."""
    if bin_bytes % 4:
        raise ValueError("the BIN chunk must be a multiple of 4 bytes long")
    text = json.dumps(doc, separators=(",", ":"), allow_nan=False).encode("ascii")
    text += b" " * (-len(text) % 4)
    return (struct.pack("<III", MAGIC, VERSION, 12 + 8 + len(text) + 8 + bin_bytes) + struct.pack("<II", len(text), CHUNK_JSON) + text
            + struct.pack("<II", bin_bytes, CHUNK_BIN))


def _per_name(value, names, what):
    """`align_to` / `move` of `write_gltf`: one value for every sequence, or a mapping from a sequence's name to its own (a name it
    does not hold: None)."""
    if isinstance(value, dict):
        if not set(value) <= set(names):
            raise ValueError("%s names sequences the file does not hold: %r" % (what, sorted(set(value) - set(names))))
        return [value.get(n) for n in names]
    return [value] * len(names)


def write_gltf(engine, sequences, path, fps=DEFAULT_FPS, align_to=None, move=None, colours=None):
    """`sequences`, an ordered mapping of name -> [F,15,3] (array or tensor, metres, equal F >= 1), as the glTF binary file `path`: one
    skinned skeleton per sequence, all keyed at every frame at `fps`.  align_to [F,15,3]: a sequence is first moved by the one
    similarity transform that takes it onto `align_to` (`errors.align_sequence`); move: a [13] device tensor (c, R, t), for instance
    `GroundEstimate.crt`, applied behind the alignment -- both for every sequence, or as a mapping name -> value for some.  colours:
    name -> (r, g, b) of 255 (default: `render.PALETTE`, else grey).  Rest lengths, meshes and animation blocks are made on the device
    into the BIN chunk as the file holds it; 19 + 6 numbers per skeleton and the counter of bad frames come back for the JSON; the
    chunk then crosses PCIe in slices of at most PINNED_BYTES through two alternating pinned buffers and is appended in order.  A frame
    with a number that is not finite (a NaN joint) raises ValueError naming the first such frame and leaves no file.  The file is
    written under a temporary name beside `path` and renamed when complete.  Runs on the current stream.  Returns F."""
    import torch
    from .render import PALETTE
    from .staging import reader_pool, stream_out
    names = list(sequences)
    if not names:
        raise ValueError("a glTF file needs at least one sequence")
    seqs = [_sequence(engine, sequences[n]) for n in names]
    F = seqs[0].shape[0]
    if any(s.shape[0] != F for s in seqs):
        raise ValueError("the sequences of a glTF file must have equally many frames, got %r" % ([int(s.shape[0]) for s in seqs],))
    if F < 1:
        raise ValueError("a glTF file needs at least one frame")
    if not (fps > 0 and np.isfinite(fps)):
        raise ValueError("fps must be positive, got %r" % (fps,))
    targets, moves = _per_name(align_to, names, "align_to"), _per_name(move, names, "move")
    table, total = section_table(names, F)
    at = {s.name: s for s in table}
    chunk = torch.zeros(total, device=engine.device, dtype=torch.uint8)          # (zeros: the padding is file content)
    counters = new_counter(engine.device).repeat(len(names), 1)
    numbers = []
    for i, (name, seq_d) in enumerate(zip(names, seqs)):
        crt = _alignment(engine, seq_d, targets[i], moves[i])
        rest = bvh.rest_lengths(engine, seq_d, crt)
        v, a = at["%s/vertices" % name], at["%s/animation" % name]
        _, bounds = rest_mesh(engine, rest, out=chunk[v.offset:v.offset + v.nbytes])
        animation(engine, seq_d, crt, fps, counters[i], out=chunk[a.offset:a.offset + a.nbytes])
        numbers.extend([rest, bounds.to(torch.float64)])
    numbers = torch.cat(numbers).cpu().numpy().reshape(len(names), 25)          # (the one read-back, with the counters behind it)
    for name, (count, first) in zip(names, counters.cpu().tolist()):
        if count:
            raise ValueError("%s: frame %d of the sequence %s has a number that is not finite (a NaN joint): no file written" % (path, first, name))
    colours = colours or {}
    doc, sections, total = build_document([(n, row[:19], row[19:], colours.get(n, PALETTE.get(n, (128, 128, 128)))) for n, row in zip(names, numbers)],
                                          F, fps)
    for s in sections:
        if s.data is not None:
            chunk[s.offset:s.offset + s.nbytes].copy_(torch.frombuffer(bytearray(s.data), dtype=torch.uint8), non_blocking=False)
    per = max(16, PINNED_BYTES // 16 * 16)
    pool = reader_pool("gltf", 1)          # one writer: the slices are appended in order

    def produce(k, out):
        n = min(per, total - k * per)
        out[:n].copy_(chunk[k * per:k * per + n])
        return n

    def consume(k, data, side):
        return [pool.submit(f.write, data.numpy())]

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = "%s.part.%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            f.write(container_head(doc, total))
            stream_out(engine.device, "gltf", per, (total + per - 1) // per, produce, consume)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return F


def release():
    """Give back the pinned and device buffers `write_gltf` keeps between calls."""
    from .staging import release_kept
    release_kept("gltf")


# ------------------------------------------------------------------------------------------------------------------ reading back
def read_glb(path):
    """A glTF binary file -> Parsed(json: the JSON chunk as a dict, accessors: every accessor's elements as a numpy array [count,
    components] (MAT4: [count,4,4], its columns as rows), bin: the BIN chunk's bytes).  Everything is checked against the lengths
    before it is read -- magic, version, the total length, the two chunks' types and lengths, every view inside the buffer, every
    accessor inside its view: ValueError otherwise.  It reads what `write_gltf` writes: one buffer, no sparse accessors."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12:
        raise ValueError("%s: %d bytes are no glTF header" % (path, len(data)))
    magic, version, length = struct.unpack_from("<III", data, 0)
    if magic != MAGIC:
        raise ValueError("%s: not a glTF binary file (magic %#x)" % (path, magic))
    if version != VERSION:
        raise ValueError("%s: glTF container version %d, not 2" % (path, version))
    if length != len(data):
        raise ValueError("%s: the header announces %d bytes, the file has %d" % (path, length, len(data)))
    chunks, at = [], 12
    while at < len(data):
        if at + 8 > len(data):
            raise ValueError("%s: a chunk header beyond the end of the file" % path)
        n, kind = struct.unpack_from("<II", data, at)
        if n % 4 or at + 8 + n > len(data):
            raise ValueError("%s: a chunk of %d bytes at %d does not fit the file's %d" % (path, n, at, len(data)))
        chunks.append((kind, data[at + 8:at + 8 + n]))
        at += 8 + n
    if len(chunks) < 1 or chunks[0][0] != CHUNK_JSON or len(chunks) > 2 or (len(chunks) == 2 and chunks[1][0] != CHUNK_BIN):
        raise ValueError("%s: wants a JSON chunk and then at most one BIN chunk" % path)
    try:
        doc = json.loads(chunks[0][1].decode("utf-8"))
    except ValueError as e:
        raise ValueError("%s: the JSON chunk does not parse: %s" % (path, e))
    blob = chunks[1][1] if len(chunks) == 2 else b""
    buffers = doc.get("buffers", [])
    if len(buffers) > 1 or (buffers and (buffers[0].get("uri") is not None or not 0 <= buffers[0].get("byteLength", -1) <= len(blob))):
        raise ValueError("%s: wants one buffer, the BIN chunk, no longer than it" % path)
    arrays = []
    for i, a in enumerate(doc.get("accessors", [])):
        try:
            v = doc["bufferViews"][a["bufferView"]]
            comps, dt = _COMPONENTS[a["type"]], np.dtype(_DTYPES[a["componentType"]])
            count, v_off, v_len = int(a["count"]), int(v.get("byteOffset", 0)), int(v["byteLength"])
        except (KeyError, IndexError, TypeError, ValueError):
            raise ValueError("%s: accessor %d is not one this reader understands" % (path, i))
        element = comps * dt.itemsize
        stride, off = int(v.get("byteStride", element)), int(a.get("byteOffset", 0))
        if v.get("buffer", 0) != 0 or v_off < 0 or v_len < 0 or v_off + v_len > buffers[0]["byteLength"]:
            raise ValueError("%s: bufferView %d lies outside the buffer" % (path, a["bufferView"]))
        if count < 0 or off < 0 or stride < element or (count and off + (count - 1) * stride + element > v_len):
            raise ValueError("%s: accessor %d lies outside its bufferView" % (path, i))
        rows = np.ndarray((count, comps), dtype=dt, buffer=blob, offset=v_off + off, strides=(stride, dt.itemsize)).copy()
        arrays.append(rows.reshape(count, 4, 4) if a["type"] == "MAT4" else rows)
    return Parsed(doc, arrays, blob)


def quaternion_matrices(q):
    """Quaternions [..., 4] (x, y, z, w) -> rotation matrices [..., 3, 3] in float64, normalised first as a player does."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def node_transforms(parsed, name):
    """Forward kinematics of the skeleton `name` of a `read_glb` result at the animation's keys -> (positions [F,19,3], global
    rotations [F,19,3,3], the indices of its 19 nodes in the file): a node's local transform is its translation -- the animated one
    where a channel drives it -- and its `rotation` channel's quaternion."""
    doc = parsed.json
    index = {n.get("name"): i for i, n in enumerate(doc["nodes"])}
    try:
        ids = [index["%s/%s" % (name, n)] for n in NODE_NAMES]
    except KeyError:
        raise ValueError("the file holds no skeleton called %s" % name)
    anim = doc["animations"][0]
    driven = {(c["target"]["node"], c["target"]["path"]): parsed.accessors[anim["samplers"][c["sampler"]]["output"]] for c in anim["channels"]}
    F = len(parsed.accessors[anim["samplers"][0]["input"]])
    parent = {c: i for i in ids for c in doc["nodes"][i].get("children", [])}
    pos, G = np.zeros((F, len(ids), 3)), np.zeros((F, len(ids), 3, 3))
    for k, i in enumerate(ids):
        t = np.asarray(driven.get((i, "translation"), np.tile(np.asarray(doc["nodes"][i].get("translation", [0.0, 0.0, 0.0])), (F, 1))), dtype=np.float64)
        R = quaternion_matrices(driven[(i, "rotation")]) if (i, "rotation") in driven else np.tile(np.eye(3), (F, 1, 1))
        if i not in parent:
            pos[:, k], G[:, k] = t, R
        else:
            p = ids.index(parent[i])
            if p >= k:
                raise ValueError("a node before its parent")
            pos[:, k] = pos[:, p] + np.einsum("nij,nj->ni", G[:, p], t)
            G[:, k] = G[:, p] @ R
    return pos, G, ids


def joint_positions(parsed, name):
    """The 15 joints of the skeleton `name` of a `read_glb` result at the animation's keys, by forward kinematics -> [F,15,3] in metres."""
    return bvh.skeleton_from_nodes(node_transforms(parsed, name)[0])


# ------------------------------------------------------------------------------------------------------------------ a result's file
def write_result(engine, path, estimated, optimized, gt=None, fps=DEFAULT_FPS, align=None, upright=None):
    """The file `path` with the skeletons `estimated`, `optimized` and, with a ground truth, `gt`, by the convention of
    `report.Outputs`: with a ground truth the first two are aligned to it (`align`, default: whenever there is one).  upright: True or
    a `ground.GroundEstimate`, as in `bvh.write_result_bvh`.  Returns the number of skeletons."""
    align = gt is not None if align is None else align
    if align and gt is None:
        raise ValueError("aligned skeletons need a ground-truth sequence to align to")
    mv, mv_gt = _upright(engine, upright, align, optimized, gt)
    sequences = {SEQUENCE_NAMES[0]: estimated, SEQUENCE_NAMES[1]: optimized}
    to = {SEQUENCE_NAMES[0]: gt, SEQUENCE_NAMES[1]: gt} if align else None
    move = {SEQUENCE_NAMES[0]: mv, SEQUENCE_NAMES[1]: mv}
    if gt is not None:
        sequences[SEQUENCE_NAMES[2]] = gt
        move[SEQUENCE_NAMES[2]] = mv_gt
    write_gltf(engine, sequences, path, fps=fps, align_to=to, move=move)
    return len(sequences)


def write_result_gltf(engine, directory, estimated, optimized, gt=None, fps=DEFAULT_FPS, align=None, upright=None):
    """`<directory>/result.glb` from the merged sequences (`write_result`).  Returns the number of skeletons in it."""
    return write_result(engine, os.path.join(directory, FILE_NAME), estimated, optimized, gt, fps=fps, align=align, upright=upright)


def main(argv=None):
    import argparse
    truthy = lambda x: str(x).lower() == "true"          # noqa: E731  (the reference's own flag parser)
    p = argparse.ArgumentParser(description="One glTF binary file of skinned, animated skeletons from a saved result_pose.pkl")
    p.add_argument("pose_pickle", help="result_pose.pkl as --save_pose writes it: estimated_pose, optimized_pose and, optionally, gt_pose")
    p.add_argument("--out", required=True, metavar="FILE.glb")
    p.add_argument("--fps", default=float(DEFAULT_FPS), type=float, help="keys per second of the animation")
    p.add_argument("--align", default=False, type=truthy, help="true: align both sequences to gt_pose first")
    p.add_argument("--upright", action="store_true", help="stand the skeletons upright on the ground estimated from the foot contacts: Y up, the floor at 0")
    p.add_argument("--foot_lock", action="store_true", help="pin the standing feet of the optimised sequence and re-solve its legs first")
    a = p.parse_args(argv)
    if not (a.fps > 0 and np.isfinite(a.fps)):
        p.error("--fps must be positive")
    n = write_result(*result_poses(p, a, "the file's meshes and animation are made on the device"), fps=a.fps, align=a.align, upright=a.upright or None)
    print("{} skeletons written to {}".format(n, a.out))


if __name__ == "__main__":
    main()
