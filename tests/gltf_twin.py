"""The numpy twin of the glTF route, float64, written from its formulas on top of the BVH twin (`frame_locals`,
`move`, `rest_lengths`, `regrow`, `joints_of`) and the mesh twin: the quaternions with their three sign rules, the animation block as
bytes, the rest-pose mesh with its skinning, linear-blend skinning of a file's mesh, and `check_container`, which holds a file's bytes
to the rules of glTF 2.0 that such a file must meet.  The container is parsed here with `struct` and `json`, not with `gltf.read_glb`."""
import json
import struct

import numpy as np

import bvh_twin as B
import mesh_twin as M

ROTATING = tuple(n for n in range(B.N) if n == 0 or B.KIDS[n])
FRAME_BYTES, VERTEX_BYTES, N_VERTICES, N_TRIANGLES = 256, 32, M.N_VERTICES, M.N_TRIANGLES
NODE_OF_JOINT = tuple(B.JOINT.index(j) for j in range(15))
TORSO_LINES, HIP_LINE = ((1, 7), (4, 11)), (7, 11)
RING_WEIGHTS = (0, 64, 128, 191, 255)
assert ROTATING == (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17)


# ------------------------------------------------------------------------------------------------------------------ quaternions
def shepperd(R):
    """One rotation matrix -> (w, x, y, z): the branch of the largest of (trace, R00, R11, R22), the first on ties."""
    t = (R[0, 0] + R[1, 1]) + R[2, 2]
    k = int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        r = np.sqrt(1.0 + t)
        return np.array([r / 2, (R[2, 1] - R[1, 2]) / (2 * r), (R[0, 2] - R[2, 0]) / (2 * r), (R[1, 0] - R[0, 1]) / (2 * r)])
    if k == 1:
        r = np.sqrt(((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2])
        return np.array([(R[2, 1] - R[1, 2]) / (2 * r), r / 2, (R[0, 1] + R[1, 0]) / (2 * r), (R[0, 2] + R[2, 0]) / (2 * r)])
    if k == 2:
        r = np.sqrt(((1.0 - R[0, 0]) + R[1, 1]) - R[2, 2])
        return np.array([(R[0, 2] - R[2, 0]) / (2 * r), (R[0, 1] + R[1, 0]) / (2 * r), r / 2, (R[1, 2] + R[2, 1]) / (2 * r)])
    r = np.sqrt(((1.0 - R[0, 0]) - R[1, 1]) + R[2, 2])
    return np.array([(R[1, 0] - R[0, 1]) / (2 * r), (R[0, 2] + R[2, 0]) / (2 * r), (R[1, 2] + R[2, 1]) / (2 * r), r / 2])


def canonical(q):
    """(w, x, y, z) with the sign that makes its first non-zero component positive."""
    for v in q:
        if v != 0:
            return -q if v < 0 else q
    return q


def canonical_quaternions(X, crt=None):
    """[F,15,3] -> (the Hips' positions [F,3], the canonical quaternions of the 15 rotating nodes [F,15,4] as (w, x, y, z))."""
    X = B.move(X, crt)
    P, c = np.empty((len(X), 3)), np.empty((len(X), len(ROTATING), 4))
    for f, x in enumerate(X):
        P[f], L = B.frame_locals(x)
        for k, n in enumerate(ROTATING):
            c[f, k] = canonical(shepperd(L[n]))
    return P, c


def continuity_signs(c):
    """[F,K,4] canonical quaternions -> s [F,K]: s[0] = +1, s[f] = -s[f-1] where c[f] . c[f-1] < 0, else s[f-1]."""
    s = np.ones(c.shape[:2])
    for f in range(1, len(c)):
        dot = (c[f] * c[f - 1]).sum(axis=-1)
        s[f] = np.where(dot < 0, -s[f - 1], s[f - 1])
    return s


def quaternions(X, crt=None):
    """The three rules: Shepperd, the canonical sign, the sign from key to key -> (P [F,3], q [F,15,4] as (w, x, y, z)), float64."""
    P, c = canonical_quaternions(X, crt)
    return P, continuity_signs(c)[..., None] * c


def matrices(q):
    """(w, x, y, z) [..., 4] -> rotation matrices [..., 3, 3], q taken as it is (no normalisation)."""
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def block_offsets(F):
    """The byte offsets of the 17 arrays of an animation block of F frames, and its size: tightly packed arrays on 16-byte starts."""
    up = lambda n: (n + 15) // 16 * 16          # noqa: E731
    off = [0, up(4 * F)]
    off.append(off[1] + up(12 * F))
    for _ in range(len(ROTATING) - 1):
        off.append(off[-1] + 16 * F)
    return off, off[-1] + 16 * F


def animation_arrays(X, crt, fps):
    """-> (times f32 [F], translation f32 [F,3], rotations f32 [15,F,4] as the file holds them: (x, y, z, w)); one rounding each."""
    P, q = quaternions(X, crt)
    times = (np.arange(len(P), dtype=np.float64) / float(fps)).astype(np.float32)
    return times, P.astype(np.float32), np.ascontiguousarray(np.transpose(q[..., [1, 2, 3, 0]], (1, 0, 2))).astype(np.float32)


def animation_block(X, crt, fps):
    times, tr, rot = animation_arrays(X, crt, fps)
    off, size = block_offsets(len(times))
    out = bytearray(size)
    for o, a in zip(off, [times, tr] + list(rot)):
        out[o:o + a.nbytes] = a.astype("<f4").tobytes()
    return bytes(out)


def parse_block(block, F):
    """The bytes of an animation block -> (times [F], translation [F,3], rotations [15,F,4]) f32, and that its padding is zero."""
    off, size = block_offsets(F)
    assert len(block) == size
    raw = np.frombuffer(bytes(block), dtype=np.uint8)
    take = lambda o, n: np.frombuffer(bytes(block), dtype="<f4", count=n, offset=o)          # noqa: E731
    assert not raw[4 * F:off[1]].any() and not raw[off[1] + 12 * F:off[2]].any(), "the padding between the arrays is zero"
    return take(off[0], F), take(off[1], 3 * F).reshape(F, 3), np.stack([take(off[2 + k], 4 * F).reshape(F, 4) for k in range(len(ROTATING))])


def turning_walker(n=130, turns=2.0):
    """`synth_walk.walk(n, seed=1)["world"]` with frame f turned about z by 2 pi turns f / (n - 1): two full turns -> [n,15,3]."""
    from globalegomocap_amd import synth_walk
    X = synth_walk.walk(n, seed=1)["world"]
    out = np.empty_like(X)
    for f in range(n):
        a = 2.0 * np.pi * turns * f / (n - 1)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out[f] = X[f] @ Rz.T
    return out


# ------------------------------------------------------------------------------------------------------------------ the rest mesh
def rest_nodes(rest):
    nodes = np.zeros((B.N, 3))
    for n in range(1, B.N):
        nodes[n] = nodes[B.PARENTS[n]] + B.REST[n] * rest[n]
    return nodes


def rest_mesh(rest):
    """The rest-pose mesh of the skeleton with the rest lengths `rest` [19] -> (positions f64 [V,3], normals f64 [V,3], JOINTS_0 u8
    [V,4], WEIGHTS_0 u8 [V,4]): the geometry of `mesh_twin.frame_mesh` on the rest joints; a sphere bound to its joint's node, a
    cylinder to the parent of its second joint's node (Hips for the hip line), a torso line's ring k (counted from its second joint, as
    the vertices are) to (second joint's node, first joint's node) with (255 - w, w); a weight of 0 names node 0."""
    joints = B.joints_of(rest_nodes(rest)[None])[0]
    pos, _, _ = M.frame_mesh(joints)
    unit, _ = M.unit_sphere()
    normals, J, W = np.zeros((N_VERTICES, 3)), np.zeros((N_VERTICES, 4), dtype=np.uint8), np.zeros((N_VERTICES, 4), dtype=np.uint8)
    for j in range(15):
        sl = slice(j * M.SPHERE_V, (j + 1) * M.SPHERE_V)
        normals[sl], J[sl, 0], W[sl, 0] = unit, NODE_OF_JOINT[j], 255
    for l, (a, b) in enumerate(M.LINES):
        v0 = 15 * M.SPHERE_V + l * M.CYLINDER_V
        with np.errstate(invalid="ignore", divide="ignore"):
            R = M.bone_rotation(joints[a], joints[b])
        local = np.zeros((M.CYLINDER_V, 3))
        local[0], local[1] = (0, 0, 1), (0, 0, -1)
        for i in range(5):
            for j in range(20):
                local[2 + 20 * i + j] = (np.cos(j * 2 * np.pi / 20), np.sin(j * 2 * np.pi / 20), 0.0)
        normals[v0:v0 + M.CYLINDER_V] = local @ R.T
        first, second = NODE_OF_JOINT[a], NODE_OF_JOINT[b]
        if (a, b) in TORSO_LINES:
            w = np.empty(M.CYLINDER_V, dtype=np.int64)
            w[0], w[1] = 0, 255
            for i in range(5):
                w[2 + 20 * i:22 + 20 * i] = RING_WEIGHTS[i]
            rows = slice(v0, v0 + M.CYLINDER_V)
            W[rows, 0], W[rows, 1] = 255 - w, w
            J[rows, 0], J[rows, 1] = np.where(255 - w > 0, second, 0), np.where(w > 0, first, 0)
        else:
            J[v0:v0 + M.CYLINDER_V, 0] = 0 if (a, b) == HIP_LINE else B.PARENTS[second]
            W[v0:v0 + M.CYLINDER_V, 0] = 255
    return pos, normals, J, W


def rest_mesh_bytes(rest):
    """-> (the 414 720 bytes of the vertex block, the bounds f32 [6] of its positions)."""
    pos, nr, J, W = rest_mesh(rest)
    rec = np.zeros(N_VERTICES, dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("j", "u1", 4), ("w", "u1", 4)]))
    rec["p"], rec["n"], rec["j"], rec["w"] = pos.astype(np.float32), nr.astype(np.float32), J, W
    return rec.tobytes(), np.concatenate([rec["p"].min(axis=0), rec["p"].max(axis=0)])


def parse_vertices(block):
    rec = np.frombuffer(bytes(block), dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("j", "u1", 4), ("w", "u1", 4)]), count=N_VERTICES)
    return rec["p"], rec["n"], rec["j"], rec["w"]


def cap_centres():
    """The vertex indices of every cylinder's two cap centres [15,2]: at the line's second joint, at its first."""
    return np.array([[15 * M.SPHERE_V + l * M.CYLINDER_V, 15 * M.SPHERE_V + l * M.CYLINDER_V + 1] for l in range(15)])


# ------------------------------------------------------------------------------------------------------------------ the container
COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
DTYPES = {5121: "u1", 5123: "<u2", 5125: "<u4", 5126: "<f4"}


def split_container(data):
    """The bytes of a .glb -> (the JSON as a dict, the BIN chunk's bytes), with the container's rules asserted."""
    assert len(data) >= 12 + 8 and data[:4] == b"glTF", "magic"
    version, length = struct.unpack_from("<II", data, 4)
    assert version == 2 and length == len(data), (version, length, len(data))
    n_json, kind = struct.unpack_from("<II", data, 12)
    assert kind == 0x4E4F534A and n_json % 4 == 0 and 20 + n_json + 8 <= len(data), "the first chunk is JSON, padded to 4"
    text = data[20:20 + n_json]
    assert text.rstrip(b" ") == text.strip() and set(text[len(text.rstrip(b" ")):]) <= {0x20}, "JSON is padded with spaces"
    n_bin, kind = struct.unpack_from("<II", data, 20 + n_json)
    assert kind == 0x004E4942 and n_bin % 4 == 0 and 28 + n_json + n_bin == len(data), "the second and last chunk is BIN, padded to 4"
    return json.loads(text.decode("utf-8")), data[28 + n_json:]


def accessor_array(doc, blob, i):
    a = doc["accessors"][i]
    v = doc["bufferViews"][a["bufferView"]]
    comps, dt = COMPONENTS[a["type"]], np.dtype(DTYPES[a["componentType"]])
    element = comps * dt.itemsize
    stride, off, count = v.get("byteStride", element), a.get("byteOffset", 0), a["count"]
    assert v["buffer"] == 0 and v.get("byteOffset", 0) >= 0 and v.get("byteOffset", 0) + v["byteLength"] <= doc["buffers"][0]["byteLength"] <= len(blob), "a view inside the buffer"
    assert count >= 1 and off + (count - 1) * stride + element <= v["byteLength"], "an accessor inside its view"
    assert (v.get("byteOffset", 0) + off) % dt.itemsize == 0 and off % dt.itemsize == 0 and stride % dt.itemsize == 0, "offsets are multiples of the component size"
    if a["type"] == "MAT4":
        assert (v.get("byteOffset", 0) + off) % 4 == 0
    return np.ndarray((count, comps), dtype=dt, buffer=blob, offset=v.get("byteOffset", 0) + off, strides=(stride, dt.itemsize)).copy()


def check_container(data):
    """Asserts the glTF 2.0 rules a file of this route must meet -> (the JSON, {accessor index: array})."""
    doc, blob = split_container(bytes(data))
    assert doc["asset"]["version"] == "2.0" and len(doc["buffers"]) == 1 and "uri" not in doc["buffers"][0]
    assert doc["buffers"][0]["byteLength"] <= len(blob) < doc["buffers"][0]["byteLength"] + 4
    arrays = {i: accessor_array(doc, blob, i) for i in range(len(doc["accessors"]))}
    views, acc, nodes = doc["bufferViews"], doc["accessors"], doc["nodes"]
    scene_nodes, todo = set(), list(doc["scenes"][doc["scene"]]["nodes"])
    while todo:
        n = todo.pop()
        assert n not in scene_nodes and 0 <= n < len(nodes), "the scene is a forest"
        scene_nodes.add(n)
        todo.extend(nodes[n].get("children", []))
    assert len(doc["meshes"]) == len(doc["skins"]) == len(doc["materials"]) >= 1
    index_accessors = set()
    for mesh in doc["meshes"]:
        assert len(mesh["primitives"]) == 1
        prim = mesh["primitives"][0]
        at = prim["attributes"]
        assert set(at) == {"POSITION", "NORMAL", "JOINTS_0", "WEIGHTS_0"} and prim.get("mode", 4) == 4 and 0 <= prim["material"] < len(doc["materials"])
        for name in at:
            v = views[acc[at[name]]["bufferView"]]
            assert v.get("byteStride") == VERTEX_BYTES and v.get("target") == 34962 and acc[at[name]]["count"] == N_VERTICES, name
        pos, a = arrays[at["POSITION"]], acc[at["POSITION"]]
        assert a["componentType"] == 5126 and a["type"] == "VEC3" and "min" in a and "max" in a
        assert np.array_equal(np.asarray(a["min"]), pos.min(axis=0).astype(np.float64)) and np.array_equal(np.asarray(a["max"]), pos.max(axis=0).astype(np.float64))
        nr = arrays[at["NORMAL"]].astype(np.float64)
        assert np.abs(np.sqrt((nr * nr).sum(axis=-1)) - 1.0).max() <= 1e-6
        assert acc[at["WEIGHTS_0"]]["componentType"] == 5121 and acc[at["WEIGHTS_0"]].get("normalized") is True
        assert (arrays[at["WEIGHTS_0"]].astype(np.int64).sum(axis=-1) == 255).all(), "WEIGHTS_0 rows sum to 255"
        assert acc[at["JOINTS_0"]]["componentType"] == 5121 and "normalized" not in acc[at["JOINTS_0"]] and (arrays[at["JOINTS_0"]] < 19).all()
        assert ((arrays[at["WEIGHTS_0"]] > 0) | (arrays[at["JOINTS_0"]] == 0)).all(), "a weight of zero names joint 0"
        ia = acc[prim["indices"]]
        index_accessors.add(prim["indices"])
        assert ia["componentType"] == 5123 and ia["type"] == "SCALAR" and ia["count"] == 3 * N_TRIANGLES
        assert views[ia["bufferView"]].get("target") == 34963 and "byteStride" not in views[ia["bufferView"]]
        assert arrays[prim["indices"]].max() < N_VERTICES
    assert len(index_accessors) == 1, "ONE index buffer"
    for skin in doc["skins"]:
        assert len(skin["joints"]) == 19 and set(skin["joints"]) <= scene_nodes and len(set(skin["joints"])) == 19, "skin joints are nodes of the scene"
        ib = acc[skin["inverseBindMatrices"]]
        assert ib["type"] == "MAT4" and ib["componentType"] == 5126 and ib["count"] == 19 and "byteStride" not in views[ib["bufferView"]]
        m = arrays[skin["inverseBindMatrices"]].reshape(19, 4, 4)          # (rows here are the matrices' columns)
        assert np.array_equal(m[:, :, 3], np.tile([0.0, 0.0, 0.0, 1.0], (19, 1))), "the last row of an inverse bind matrix is (0, 0, 0, 1)"
    skinned = [n for n in range(len(nodes)) if "mesh" in nodes[n]]
    assert len(skinned) == len(doc["meshes"]) and all("skin" in nodes[n] and n in doc["scenes"][doc["scene"]]["nodes"] for n in skinned)
    assert len(doc["animations"]) == 1, "ONE animation"
    anim = doc["animations"][0]
    inputs = {s["input"] for s in anim["samplers"]}
    assert len(inputs) == 1, "the key times are shared"
    ta = acc[next(iter(inputs))]
    times = arrays[next(iter(inputs))][:, 0]
    assert ta["componentType"] == 5126 and ta["type"] == "SCALAR" and ta["min"] == [float(times.min())] and ta["max"] == [float(times.max())]
    assert times[0] == 0 and (np.diff(times.astype(np.float64)) > 0).all(), "times strictly increasing"
    targets = set()
    for ch in anim["channels"]:
        s, t = anim["samplers"][ch["sampler"]], ch["target"]
        assert s.get("interpolation", "LINEAR") == "LINEAR" and t["node"] in scene_nodes and (t["node"], t["path"]) not in targets
        targets.add((t["node"], t["path"]))
        oa, out = acc[s["output"]], arrays[s["output"]]
        assert "byteStride" not in views[oa["bufferView"]] and "target" not in views[oa["bufferView"]], "no stride on animation data"
        assert oa["count"] == ta["count"] and oa["componentType"] == 5126 and oa["type"] == {"translation": "VEC3", "rotation": "VEC4"}[t["path"]]
        assert np.isfinite(out).all()
        if t["path"] == "rotation":
            q = out.astype(np.float64)
            assert np.abs(np.sqrt((q * q).sum(axis=-1)) - 1.0).max() <= 1e-6, "unit quaternions"
    assert len(targets) == 16 * len(doc["skins"])
    return doc, arrays


def assemble(doc, sections, total, made):
    """A file's bytes from `gltf.build_document`'s results; made: section name -> bytes for the sections the device makes."""
    from globalegomocap_amd import gltf
    blob = bytearray(total)
    for s in sections:
        data = s.data if s.data is not None else made[s.name]
        assert len(data) == s.nbytes and s.offset % 16 == 0
        blob[s.offset:s.offset + s.nbytes] = data
    return gltf.container_head(doc, total) + bytes(blob)


# ------------------------------------------------------------------------------------------------------------------ skinning
def skin(parsed, name, f):
    """Linear-blend skinning of the mesh of skeleton `name` of a `gltf.read_glb` result at key f -> positions f64 [V,3]: every
    vertex moved by sum_i w_i G(joint_i) inverse_bind(joint_i), G the nodes' global transforms by this module's own forward kinematics."""
    doc, acc = parsed.json, parsed.accessors
    mesh_node = next(n for n in doc["nodes"] if n.get("name") == name and "mesh" in n)
    skin_ = doc["skins"][mesh_node["skin"]]
    at = doc["meshes"][mesh_node["mesh"]]["primitives"][0]["attributes"]
    pos, J, W = acc[at["POSITION"]].astype(np.float64), acc[at["JOINTS_0"]], acc[at["WEIGHTS_0"]].astype(np.float64) / 255.0
    ibm = np.transpose(acc[skin_["inverseBindMatrices"]].astype(np.float64).reshape(-1, 4, 4), (0, 2, 1))          # column-major -> matrices
    anim = doc["animations"][0]
    driven = {(c["target"]["node"], c["target"]["path"]): acc[anim["samplers"][c["sampler"]]["output"]][f].astype(np.float64) for c in anim["channels"]}
    parent = {c: i for i, n in enumerate(doc["nodes"]) for c in n.get("children", [])}
    G = {}

    def world(i):
        if i not in G:
            n = doc["nodes"][i]
            T = np.eye(4)
            T[:3, 3] = driven.get((i, "translation"), np.asarray(n.get("translation", [0.0, 0.0, 0.0])))
            if (i, "rotation") in driven:
                x, y, z, w = driven[(i, "rotation")]
                q = np.array([w, x, y, z])
                T[:3, :3] = matrices(q / np.sqrt(q @ q))
            G[i] = world(parent[i]) @ T if i in parent else T
        return G[i]
    mats = np.stack([world(j) @ ibm[k] for k, j in enumerate(skin_["joints"])])
    hom = np.concatenate([pos, np.ones((len(pos), 1))], axis=1)
    out = np.zeros((len(pos), 3))
    for slot in range(4):
        out += W[:, slot:slot + 1] * np.einsum("vij,vj->vi", mats[J[:, slot]], hom)[:, :3]
    return out
