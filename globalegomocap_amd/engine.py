"""Thin Python object over the C ABI: owns one `gem_handle`, hands torch device pointers to it.

PyTorch is used for device memory and streams only; every number of the path is produced by the
HIP kernels behind `libgem_hip.so`.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._binding import _ptr, _stream, check_tensor, check_tensors          # noqa: F401 (_ptr, _stream: the tests' way in)
from .camera import FisheyeCamera, DEFAULT_CALIBRATION
from .skeleton import KINEMATIC_PARENTS, N_JOINTS
from .vae import VAEShape, flatten_state_dict

LOCAL_STAGE, GLOBAL_STAGE = _capi.STAGE_LOCAL, _capi.STAGE_GLOBAL


def _check_seq_crt(what, frames, seq, crt):
    """What `skeleton_mesh`, `skeleton_capsules` and `project_sequence` ask of their sequence [`frames`,15,3] f64 and of the (c, R, t) it
    is moved by, where one is given."""
    check_tensor(seq, torch.float64, error=TypeError("%s wants a contiguous float64 device tensor" % what))
    check_tensor(seq, torch.float64, (None, N_JOINTS, 3),
                 error=ValueError("%s: seq must be [%s,%d,3], got %s" % (what, frames, N_JOINTS, tuple(seq.shape))))
    if crt is not None:
        check_tensor(crt, torch.float64, numel=13, error=TypeError("%s: crt must be a contiguous float64 device tensor of 13 values" % what))


def energy_weights(w3d, smooth, bone, vae, reproj):
    return _capi.GemEnergyWeights(float(w3d), float(smooth), float(bone), float(vae), float(reproj))


class WindowEngine:
    """B independent windows per call; one engine per device."""

    def __init__(self, shape=None, camera=None, max_windows=256, heat_size=(64, 64), device=None):
        self.lib = _capi.load_library()
        if not torch.cuda.is_available():
            raise _capi.GemError("no HIP device visible: the window optimiser has no CPU path")
        self.shape = shape or VAEShape()
        self.camera = camera or FisheyeCamera.from_json(DEFAULT_CALIBRATION)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.max_windows = int(max_windows)
        self.heat_size = tuple(heat_size)
        cfg = _capi.GemConfig()
        cfg.seq_len, cfg.n_joints, cfg.latent_dim = self.shape.seq_len, N_JOINTS, self.shape.latent_dim
        cfg.n_hidden = len(self.shape.hidden)
        for i, v in enumerate(self.shape.hidden):
            cfg.hidden[i] = v
        cfg.heat_h, cfg.heat_w = self.heat_size
        cfg.n_poly = len(self.camera.poly_w2c)
        for i, v in enumerate(self.camera.poly_w2c):
            cfg.poly[i] = v
        cfg.cx, cfg.cy = self.camera.cx, self.camera.cy
        for i, v in enumerate(KINEMATIC_PARENTS):
            cfg.parents[i] = v
        cfg.max_windows, cfg.device = self.max_windows, self.device.index
        self._h = C.c_void_p()
        _capi.check(self.lib.gem_create(C.byref(cfg), C.byref(self._h)), self.lib)
        self.T, self.D = self.shape.seq_len, self.shape.latent_dim
        self.precision = "f32"
        self._graphs, self._gstream, self._bufs = False, None, {}
        self._pinned = {}          # graph mode: signature (input addresses) -> the caller's input tensors, kept alive (see _pin)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_texel_cache(self, on=True):
        """Diagnostic switch of the reprojection term's texel-block cache (gem_set_texel_cache); results do not depend on it."""
        _capi.check(self.lib.gem_set_texel_cache(self._h, 1 if on else 0), self.lib)

    def enable_graphs(self, on=True):
        """hipGraph replay of whole `optimize_windows` / `optimize_stage` calls (gem_graph_enable): the first call with a
        given signature runs eagerly, the second is captured, later ones are ONE graph launch instead of ~700 kernel launches.
        With graphs on, the calls run on a stream owned by the engine (the legacy default stream cannot be captured; the
        caller's current stream waits for it) and their OUTPUT tensors are engine-owned buffers that the next call with the
        same batch size overwrites -- which is what keeps the signature (all pointers) stable.  Inputs must be the same
        tensors from call to call to get replays."""
        _capi.check(self.lib.gem_graph_enable(self._h, 1 if on else 0), self.lib)
        self._graphs = bool(on)
        if not on:
            self._pinned.clear()          # (gem_graph_enable(0) dropped the captured calls)
        if on and self._gstream is None:
            self._gstream = torch.cuda.Stream(device=self.device)

    MAX_PINNED = 4

    def drop_graphs(self):
        """Forget every captured call (gem_graph_enable 0 / 1: synchronises the device) and release the input tensors they pinned."""
        _capi.check(self.lib.gem_graph_enable(self._h, 0), self.lib)
        if self._graphs:
            _capi.check(self.lib.gem_graph_enable(self._h, 1), self.lib)
        self._pinned.clear()

    def _pin(self, *tensors):
        """A captured call holds the ADDRESSES of the caller's input tensors.  If the caller freed them, a later tensor could land on
        the same addresses and the old graph would be replayed on it -- on ROCm 7.2 that ended in a GPU memory fault even for
        equally sized buffers.  So the engine keeps the inputs of every signature it has seen alive (at most
        MAX_PINNED distinct input sets; one more drops all graphs and pins).  `drop_graphs()` releases them explicitly."""
        if not self._graphs:
            return
        key = tuple(t.data_ptr() for t in tensors if t is not None)
        if key not in self._pinned:
            if len(self._pinned) >= self.MAX_PINNED:
                self.drop_graphs()
            self._pinned[key] = tensors

    def graph_stats(self):
        c, r = C.c_int64(), C.c_int64()
        _capi.check(self.lib.gem_graph_stats(self._h, C.byref(c), C.byref(r)), self.lib)
        return {"captures": c.value, "replays": r.value}

    def _out(self, key, shape, dtype, zero=False):
        """Output buffer: fresh per call, or (graphs on) one persistent buffer per (entry point, role, shape)."""
        if not self._graphs:
            return (torch.zeros if zero else torch.empty)(shape, device=self.device, dtype=dtype)
        k = (key, tuple(shape), dtype)
        if k not in self._bufs:
            self._bufs[k] = torch.zeros(shape, device=self.device, dtype=dtype)
        return self._bufs[k]

    def _staged(self, key, t):
        """Copy of `t` in a persistent engine-owned buffer (graph mode: stable pointers for per-call temporaries)."""
        buf = self._out(key, tuple(t.shape), t.dtype)
        buf.copy_(t)
        return buf

    def _call(self, fn):
        """Run fn(stream_ptr) on the caller's current stream, or (graphs on) on the engine's stream, ordered after
        everything already enqueued on the current stream and before everything enqueued on it afterwards."""
        if not self._graphs:
            return fn(_stream())
        cur = torch.cuda.current_stream()
        self._gstream.wait_stream(cur)
        with torch.cuda.stream(self._gstream):
            r = fn(C.c_void_p(self._gstream.cuda_stream))
        cur.wait_stream(self._gstream)
        return r

    def set_lanes(self, min_windows):
        """Accepted for compatibility (gem_set_lanes): every optimize_windows call runs as one lane whatever `min_windows` (>= 0).
        The two-lane schedule it used to switch on measured slower than one lane and is no longer in the library."""
        _capi.check(self.lib.gem_set_lanes(self._h, int(min_windows)), self.lib)

    def set_precision(self, mode):
        """'f32' (default) | 'bf16x3' (split-bf16 MFMA, fp32-grade) | 'bf16' for the wide decoder/encoder products."""
        _capi.check(self.lib.gem_set_precision(self._h, _capi.PRECISION[mode]), self.lib)
        self.precision = mode

    # ------------------------------------------------------------------ weights
    def load_vae(self, stage, state_dict):
        blobs = flatten_state_dict(state_dict, self.shape)
        n = len(blobs)
        ptrs = (C.c_void_p * n)(*[b.ctypes.data_as(C.c_void_p) for b in blobs])
        sizes = (C.c_int64 * n)(*[b.size for b in blobs])
        _capi.check(self.lib.gem_load_vae(self._h, stage, n, ptrs, sizes), self.lib)

    # ------------------------------------------------------------------ helpers
    def _f32(self, a, shape=None):
        t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if shape is not None:
            t = t.reshape(shape)
        return t

    def _i32(self, a):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=self.device, dtype=torch.int32).contiguous()

    def _check_B(self, B):
        if B > self.max_windows:
            raise ValueError("B=%d exceeds max_windows=%d of this engine" % (B, self.max_windows))

    def _check_heat(self, heat_t, frame0, B):
        """Heat-map resolution and window starts against the frames actually held (the C ABI never learns n_frames: a wrong
        start would be a silent out-of-bounds read on the device).  frame0 is checked when it is host data (no sync)."""
        if heat_t is None:
            return
        if heat_t.dim() != 4 or tuple(heat_t.shape[1:]) != (self.heat_size[0], self.heat_size[1], N_JOINTS):
            raise ValueError("heat-maps must be [F,%d,%d,%d] (the engine's heat_size), got %s"
                             % (self.heat_size[0], self.heat_size[1], N_JOINTS, tuple(heat_t.shape)))
        if frame0 is None:
            raise ValueError("heat-maps need the first frame of every window (frame0)")
        if not torch.is_tensor(frame0) or not frame0.is_cuda:
            f = np.asarray(frame0.cpu() if torch.is_tensor(frame0) else frame0).reshape(-1)
            if f.shape[0] != B:
                raise ValueError("frame0 has %d entries for %d windows" % (f.shape[0], B))
            if B and (f.min() < 0 or f.max() + self.T > heat_t.shape[0]):
                raise ValueError("a window [frame0, frame0 + %d) leaves the %d frames of heat-maps" % (self.T, heat_t.shape[0]))

    def mean_bone_length(self, poses):
        p = self._f32(poses).reshape(-1, N_JOINTS, 3)
        out = torch.empty(N_JOINTS, device=self.device, dtype=torch.float32)
        _capi.check(self.lib.gem_mean_bone_length(self._h, _ptr(p), p.shape[0], _ptr(out), _stream()), self.lib)
        return out

    def encode(self, stage, pose, eps=None):
        pose = self._f32(pose).reshape(-1, self.T, N_JOINTS * 3)
        B = pose.shape[0]
        self._check_B(B)
        eps_t = self._f32(eps).reshape(B, self.D) if eps is not None else None
        mu, lv, z = (torch.empty(B, self.D, device=self.device) for _ in range(3))
        _capi.check(self.lib.gem_encode(self._h, stage, B, _ptr(pose), _ptr(eps_t), _ptr(mu), _ptr(lv), _ptr(z), _stream()),
                    self.lib)
        return mu, lv, z

    def decode(self, stage, z):
        z = self._f32(z).reshape(-1, self.D)
        B = z.shape[0]
        self._check_B(B)
        out = torch.empty(B, self.T, N_JOINTS, 3, device=self.device)
        _capi.check(self.lib.gem_decode(self._h, stage, B, _ptr(z), _ptr(out), _stream()), self.lib)
        return out

    def energy_grad(self, stage, z, pose_init, mean_bone, weights, heat=None, frame0=None):
        z = self._f32(z).reshape(-1, self.D)
        B = z.shape[0]
        self._check_B(B)
        p0 = self._f32(pose_init).reshape(B, self.T, N_JOINTS, 3)
        mb = self._f32(mean_bone).reshape(-1, N_JOINTS).expand(B, N_JOINTS).contiguous()
        heat_t = self._f32(heat) if heat is not None else None
        f0 = self._i32(frame0) if frame0 is not None else None
        self._check_heat(heat_t, frame0, B)
        E = torch.empty(B, device=self.device, dtype=torch.float64)
        parts = torch.empty(B, 5, device=self.device, dtype=torch.float64)
        dz = torch.empty(B, self.D, device=self.device)
        X = torch.empty(B, self.T, N_JOINTS, 3, device=self.device)
        _capi.check(self.lib.gem_energy_grad(self._h, stage, B, _ptr(z), _ptr(p0), _ptr(heat_t), _ptr(f0), _ptr(mb),
                                             C.byref(weights), _ptr(E), _ptr(parts), _ptr(dz), _ptr(X), _stream()), self.lib)
        return E, parts, dz, X

    def optimize_stage(self, stage, pose_in, mean_bone, eps, weights, heat=None, frame0=None, opts=None, want_stats=True):
        """One stage for B windows.  With graphs on, the small inputs (pose, mean bone, eps, frame0) are copied into
        engine-owned buffers so that the call's signature is stable from call to call (replay needs identical pointers);
        `heat` is passed through as it is and must be the same device tensor to get replays.  Outputs are kept per stage."""
        p = self._f32(pose_in).reshape(-1, self.T, N_JOINTS, 3)
        B = p.shape[0]
        self._check_B(B)
        mb = self._f32(mean_bone).reshape(-1, N_JOINTS).expand(B, N_JOINTS).contiguous()
        eps_t = self._f32(eps).reshape(B, self.D)
        heat_t = self._f32(heat) if heat is not None else None
        f0 = self._i32(frame0) if frame0 is not None else None
        self._check_heat(heat_t, frame0, B)
        if self._graphs:
            p, mb, eps_t = (self._staged("stage%d_%s" % (stage, k), t) for k, t in (("pose", p), ("mb", mb), ("eps", eps_t)))
            f0 = self._staged("stage%d_f0" % stage, f0) if f0 is not None else None
            self._pin(heat_t)
        opts = opts or _capi.default_lbfgs_opts()
        out = self._out("stage%d_out" % stage, (B, self.T, N_JOINTS, 3), torch.float32)
        stats = self._out("stage%d_stats" % stage, (B, 4), torch.int32, zero=True) if want_stats else None
        self._call(lambda st: _capi.check(self.lib.gem_optimize_stage(self._h, stage, B, _ptr(p), _ptr(heat_t), _ptr(f0), _ptr(mb),
                                                                      _ptr(eps_t), C.byref(weights), C.byref(opts), _ptr(out),
                                                                      _ptr(stats), st), self.lib))
        return out, stats

    def optimize_windows(self, local_pose, cams, heat, frame0, mean_bone, eps_local, eps_global, w_local, w_global,
                         opts=None, want_stats=True):
        """All tensors must already live on the device (this is the timed call of bench.py).

        local_pose [F,15,3] f32, cams [F,4,4] f64, heat [F,H,W,15] f32, frame0 [B] i32, mean_bone [B,15] f32,
        eps_* [B,D] f32 -> (mid_local [B,T,15,3] f32, global [B,T,15,3] f64, stats [2B,4] i32 or None)."""
        B = frame0.shape[0]
        self._check_B(B)
        for t, dt in ((local_pose, torch.float32), (cams, torch.float64), (heat, torch.float32), (frame0, torch.int32),
                      (mean_bone, torch.float32), (eps_local, torch.float32), (eps_global, torch.float32)):
            if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
                raise TypeError("optimize_windows wants contiguous device tensors of the documented dtypes")
        F = local_pose.shape[0]
        if cams.shape[0] != F or (heat is not None and heat.shape[0] != F):
            raise ValueError("optimize_windows: local_pose, cams and heat must cover the same frames (%d / %d / %s)"
                             % (F, cams.shape[0], None if heat is None else heat.shape[0]))
        if tuple(local_pose.shape[1:]) != (N_JOINTS, 3) or tuple(cams.shape[1:]) != (4, 4):
            raise ValueError("optimize_windows: local_pose must be [F,15,3] and cams [F,4,4]")
        if heat is not None and tuple(heat.shape[1:]) != (self.heat_size[0], self.heat_size[1], N_JOINTS):
            raise ValueError("optimize_windows: heat-maps must be [F,%d,%d,%d] (the engine's heat_size), got %s"
                             % (self.heat_size[0], self.heat_size[1], N_JOINTS, tuple(heat.shape)))
        if tuple(mean_bone.shape) != (B, N_JOINTS) or tuple(eps_local.shape) != (B, self.D) or tuple(eps_global.shape) != (B, self.D):
            raise ValueError("optimize_windows: mean_bone must be [B,15] and eps_* [B,%d] with B = %d windows" % (self.D, B))
        if F < self.T:
            raise ValueError("optimize_windows: %d frames cannot hold a %d-frame window" % (F, self.T))
        opts = opts or _capi.default_lbfgs_opts()
        self._pin(local_pose, cams, heat, frame0, mean_bone, eps_local, eps_global)
        mid = self._out("win_mid", (B, self.T, N_JOINTS, 3), torch.float32)
        glob = self._out("win_glob", (B, self.T, N_JOINTS, 3), torch.float64)
        stats = self._out("win_stats", (2 * B, 4), torch.int32, zero=True) if want_stats else None
        self._call(lambda st: _capi.check(self.lib.gem_optimize_windows(self._h, B, _ptr(local_pose), _ptr(cams), _ptr(heat),
                                                                        _ptr(frame0), _ptr(mean_bone), _ptr(eps_local),
                                                                        _ptr(eps_global), C.byref(w_local), C.byref(w_global),
                                                                        C.byref(opts), _ptr(mid), _ptr(glob), _ptr(stats), st),
                                          self.lib))
        return mid, glob, stats

    def read_trace(self, B, n_rounds=33):
        """Closure values of the last stage run on this engine: numpy [B, n_rounds] f64, NaN after a window's last
        evaluation (column r = evaluation round r).  For parity tests against the reference's closure traces."""
        self._check_B(B)
        out = torch.empty(n_rounds, B, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_read_trace(self._h, B, n_rounds, _ptr(out), _stream()), self.lib)
        return out.cpu().numpy().T.copy()

    # ------------------------------------------------------------------ the L-BFGS kernels stepped alone (parity tests)
    def lbfgs_debug_begin(self, x0, slots=0):
        """Start B = x0.shape[0] solvers at x0 [B,D] (gem_lbfgs_debug_begin); slots: 0 no slot table, 1 compact_kernel between
        the rounds, 2 slots handed out by lbfgs_advance.  Needs no weights; a test hook, not part of the reference's surface."""
        x0 = self._f32(x0).reshape(-1, self.D)
        self._check_B(x0.shape[0])
        _capi.check(self.lib.gem_lbfgs_debug_begin(self._h, x0.shape[0], _ptr(x0), int(slots), _stream()), self.lib)

    def lbfgs_debug_advance(self, f, g, opts=None, n_slabs=0):
        """One evaluation round: f [B] f64 by window, g [max(n_slabs,1),B,D] f32 with window b's row at slot_of[b]."""
        f = torch.as_tensor(f).to(device=self.device, dtype=torch.float64).contiguous()
        B = f.shape[0]
        self._check_B(B)
        g = self._f32(g)
        if g.numel() != max(int(n_slabs), 1) * B * self.D:
            raise ValueError("lbfgs_debug_advance: g must be [max(n_slabs,1), %d, %d]" % (B, self.D))
        opts = opts or _capi.default_lbfgs_opts()
        _capi.check(self.lib.gem_lbfgs_debug_advance(self._h, B, C.byref(opts), _ptr(f), _ptr(g), int(n_slabs), _stream()), self.lib)

    def lbfgs_debug_read(self, B):
        """State of the B solvers (gem_lbfgs_debug_read): dict with one numpy array [B] per field of gem_lbfgs_debug_state,
        device tensors x, d, trial [B,D] (bf16 precision: trial is the bf16 trial point widened), slot_of [B] and count of the
        next advance call."""
        self._check_B(B)
        words = C.sizeof(_capi.GemLbfgsDebugState) // 8
        st = torch.zeros(B, words, device=self.device, dtype=torch.int64)
        x, d, trial = (torch.empty(B, self.D, device=self.device) for _ in range(3))
        slot_of = torch.empty(B, device=self.device, dtype=torch.int32)
        count = torch.empty(1, device=self.device, dtype=torch.int32)
        _capi.check(self.lib.gem_lbfgs_debug_read(self._h, B, _ptr(st), _ptr(x), _ptr(d), _ptr(trial), _ptr(slot_of), _ptr(count),
                                                  _stream()), self.lib)
        raw = st.cpu().numpy()
        ints, dbl = raw[:, :6].copy().view(np.int32), raw[:, 6:].copy().view(np.float64)
        out = {k: ints[:, i].copy() for i, k in enumerate(n for n, _ in _capi.GemLbfgsDebugState._fields_[:12])}
        out.update({k: dbl[:, i].copy() for i, k in enumerate(n for n, _ in _capi.GemLbfgsDebugState._fields_[12:])})
        out.update(x=x, d=d, trial=trial, slot_of=slot_of.cpu().numpy(), count=int(count.item()))
        return out

    # ------------------------------------------------------------------ one layer through a GEMM dispatch function (parity tests)
    def gemm_debug_layer(self, w, bias):
        """A stand-alone layer from host weights w [taps,N,K] and bias [N], padded (gem_gemm_debug_layer_create): the handle to
        give `gemm_debug_run`.  Freed by `gemm_debug_layer_free` or with the engine."""
        w = np.ascontiguousarray(w, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        if w.ndim != 3 or bias.shape != (w.shape[1],):
            raise ValueError("gemm_debug_layer: w must be [taps,N,K] and bias [N]")
        out = C.c_void_p()
        _capi.check(self.lib.gem_gemm_debug_layer_create(self._h, w.shape[0], w.shape[1], w.shape[2], w.ctypes.data_as(C.c_void_p),
                                                         bias.ctypes.data_as(C.c_void_p), C.byref(out)), self.lib)
        return out

    def gemm_debug_layer_free(self, layer):
        _capi.check(self.lib.gem_gemm_debug_layer_destroy(self._h, layer), self.lib)

    def gemm_debug_run(self, layer, A, C_out, M, epi, route=0, T=1, aux=None, rows=None, row_map=None, defer=False, out_bf16=False,
                       allow_split=False, family=-1):
        """One layer through launch_gemm (route 0) or gemm_bf16a (route 1) (gem_gemm_debug_run): A [a_rows,K] f32, C_out [>=M,N]
        f32 (or bf16 storage), aux [M,N] f32, rows int32 {m, m*T}, row_map int32 [M], all device tensors.  Returns (kernel
        names, info) with info = (slabs left to the consumer, workgroups of a device-side cut, 1 if C_out holds bf16)."""
        a = _capi.GemGemmDebugArgs(route=int(route), epi=int(epi), M=int(M), T=int(T), a_rows=int(A.shape[0]), family=int(family),
                                   out_bf16=int(bool(out_bf16)), allow_split=int(bool(allow_split)), defer=int(bool(defer)), reserved=0,
                                   d_A=A.data_ptr(), d_aux=aux.data_ptr() if aux is not None else None, d_C=C_out.data_ptr(),
                                   d_rows=rows.data_ptr() if rows is not None else None,
                                   d_row_map=row_map.data_ptr() if row_map is not None else None)
        names = C.create_string_buffer(2048)
        info = (C.c_int32 * 4)()
        _capi.check(self.lib.gem_gemm_debug_run(self._h, layer, C.byref(a), names, len(names), info, _stream()), self.lib)
        return [n for n in names.value.decode().split("; ") if n], tuple(info)[:3]

    # ------------------------------------------------------------------ sequence post-processing
    def _f64(self, a):
        t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
        return t.to(device=self.device, dtype=torch.float64).contiguous()

    def merge_windows(self, windows, n_chunks, overlap=2, smooth=True):
        """merge_batches per chunk (+ gaussian_filter1d sigma=1 per chunk): [n_chunks*wpc,T,J,3] -> [n_chunks*fpc,J,3] f64."""
        w = self._f64(windows).reshape(-1, self.T, N_JOINTS, 3)
        if n_chunks < 1 or w.shape[0] % n_chunks:
            raise ValueError("merge_windows: %d windows do not split into %d chunks" % (w.shape[0], n_chunks))
        wpc = w.shape[0] // n_chunks
        fpc = wpc * (self.T - overlap) + overlap
        out = torch.empty(n_chunks * fpc, N_JOINTS, 3, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_merge_windows(self._h, _ptr(w), n_chunks, wpc, overlap, 1 if smooth else 0, _ptr(out), _stream()),
                    self.lib)
        return out

    ERROR_KEYS = ("original_global_mpjpe", "mid_global_mpjpe", "optimized_global_mpjpe", "original_camera_pos_error",
                  "optimized_camera_pos_error", "original_aligned_camera_pos_error", "mid_aligned_camera_pose_error",
                  "optimized_aligned_camera_pos_error", "original_aligned_global_mpjpe", "aligned_mid_seq_mpjpe",
                  "optimized_aligned_global_mpjpe", "aligned_original_mpjpe", "aligned_mid_optimized_mpjpe",
                  "aligned_optimized_mpjpe", "bone_length_aligned_original_mpjpe", "bone_length_aligned_mid_optimized_mpjpe",
                  "bone_length_aligned_optimized_mpjpe")

    def calculate_errors_device(self, est, mid, opt, gt):
        """calculate_errors on the device: returns the [17+J] f64 tensor (no synchronisation)."""
        from .skeleton import mean_bone_length_mm
        e, m, o, g = (self._f64(x).reshape(-1, N_JOINTS, 3) for x in (est, mid, opt, gt))
        if not (e.shape == m.shape == o.shape == g.shape):
            raise AssertionError("calculate_errors: sequences differ in shape")
        bone = np.ascontiguousarray(mean_bone_length_mm(), dtype=np.float64)
        out = torch.empty(17 + N_JOINTS, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_calculate_errors(self._h, _ptr(e), _ptr(m), _ptr(o), _ptr(g), e.shape[0],
                                                  bone.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out), _stream()), self.lib)
        return out

    def calculate_errors_chunks(self, est, mid, opt, gt, n_chunks):
        """calculate_errors for each of `n_chunks` equally long sequences laid end to end (device f64 tensors [n_chunks*F,J,3]):
        [n_chunks, 17+J] f64 on the device, one library call, no synchronisation."""
        from .skeleton import mean_bone_length_mm
        wrong = TypeError("calculate_errors_chunks wants equally shaped contiguous float64 device tensors")
        check_tensor(est, torch.float64, error=wrong)
        for x in (mid, opt, gt):
            check_tensor(x, torch.float64, tuple(est.shape), error=wrong)
        total = est.numel() // (N_JOINTS * 3)
        if n_chunks < 1 or total % n_chunks:
            raise ValueError("calculate_errors_chunks: %d frames do not split into %d chunks" % (total, n_chunks))
        bone = np.ascontiguousarray(mean_bone_length_mm(), dtype=np.float64)
        out = torch.empty(n_chunks, 17 + N_JOINTS, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_calculate_errors_chunks(self._h, _ptr(est), _ptr(mid), _ptr(opt), _ptr(gt), n_chunks, total // n_chunks,
                                                         bone.ctypes.data_as(C.POINTER(C.c_double)), _ptr(out), _stream()), self.lib)
        return out

    QUALITY_KEYS = ("heatmap_response", "bone_length_rms", "acceleration", "displacement")

    def sequence_quality(self, seq, cams, heat, frame0, mean_bone, n_chunks, ref=None):
        """The report that needs no ground truth (gem_sequence_quality) for `n_chunks` equally long merged sequences laid end to end:
        seq (and ref, optional) [n_chunks*fpc,J,3] f64, cams [F,4,4] f64 and heat [F,H,W,J] f32 the frame buffers, frame0 [n_chunks]
        i64 each chunk's first frame in them, mean_bone [n_chunks,J] f32 -- contiguous device tensors.  -> [n_chunks,4] f64 on the
        device in the order of QUALITY_KEYS (displacement NaN without `ref`), one library call, no synchronisation."""
        check_tensors("sequence_quality", (seq, torch.float64, None), (ref, torch.float64, None), (cams, torch.float64, None),
                      (heat, torch.float32, None), (frame0, torch.int64, None), (mean_bone, torch.float32, None))
        total = seq.numel() // (N_JOINTS * 3)
        if n_chunks < 1 or total % n_chunks or total == 0 or seq.numel() != total * N_JOINTS * 3:
            raise ValueError("sequence_quality: %d frames do not split into %d chunks" % (total, n_chunks))
        if ref is not None and ref.shape != seq.shape:
            raise ValueError("sequence_quality: ref must have the shape of seq")
        F = cams.shape[0]
        if tuple(cams.shape[1:]) != (4, 4) or tuple(heat.shape) != (F, self.heat_size[0], self.heat_size[1], N_JOINTS):
            raise ValueError("sequence_quality: cams must be [F,4,4] and heat [F,%d,%d,%d] over the same frames" % (self.heat_size + (N_JOINTS,)))
        if tuple(frame0.shape) != (n_chunks,) or tuple(mean_bone.shape) != (n_chunks, N_JOINTS):
            raise ValueError("sequence_quality: frame0 must be [%d] and mean_bone [%d,%d]" % (n_chunks, n_chunks, N_JOINTS))
        out = torch.empty(n_chunks, 4, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_sequence_quality(self._h, _ptr(seq), _ptr(cams), _ptr(heat), F, _ptr(frame0), _ptr(mean_bone), _ptr(ref),
                                                  n_chunks, total // n_chunks, _ptr(out), _stream()), self.lib)
        return out

    def sequence_align(self, src, dst):
        """The similarity of `errors.align_sequence` / the reference's global_align_skeleton_seq on the device (gem_sequence_align):
        src, dst [F,J,3] (or [N,3]) f64 contiguous device tensors of one shape -> [13] f64 on the device: c, R (row-major), t with
        dst ~ c * (src @ R) + t.  No synchronisation; the same bits on every call."""
        for x in (src, dst):
            check_tensor(x, torch.float64, error=TypeError("sequence_align wants contiguous float64 device tensors"))
        if src.shape != dst.shape or src.numel() == 0 or src.shape[-1] != 3:
            raise ValueError("sequence_align: src and dst must be equally shaped, non-empty [...,3], got %s and %s" % (tuple(src.shape), tuple(dst.shape)))
        out = torch.empty(13, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_sequence_align(_ptr(src), _ptr(dst), src.numel() // 3, _ptr(out), _stream()), self.lib)
        return out

    def skeleton_mesh(self, seq, crt=None, out=None):
        """The vertex blocks of the skeleton meshes of `seq` [F,J,3] f64 (contiguous device tensor), every joint moved by `crt`
        ([13] from `sequence_align`) first when given (gem_skeleton_mesh) -> uint8 [F, stride] on the device, `out` when given (its
        row stride is the frame stride: at least the vertex block, a multiple of 16, 16-byte aligned rows).  No synchronisation."""
        from . import meshes
        _check_seq_crt("skeleton_mesh", "F", seq, crt)
        F, block = seq.shape[0], meshes.layout().vertex_bytes
        if out is None:
            out = torch.empty(F, block, device=self.device, dtype=torch.uint8)
        check_tensor(out, torch.uint8, rows=(F, block),
                     error=ValueError("skeleton_mesh: out must be a uint8 device tensor [%d, >= %d] with contiguous rows" % (F, block)))
        _capi.check(self.lib.gem_skeleton_mesh(_ptr(seq), F, _ptr(crt), _ptr(out), out.stride(0), _stream()), self.lib)
        return out

    def skeleton_capsules(self, seq, crt=None, rgb_joint=0, rgb_line=0):
        """The 30 capsules of every frame of `seq` [F,J,3] f64 (contiguous device tensor), behind `crt` ([13] from `sequence_align`)
        when given (gem_skeleton_capsules): geometry [F*30,7] f64 (a, b, r) and colours [F*30] int32 (0x00BBGGRR; `rgb_joint` for the
        15 joints, `rgb_line` for the 15 lines), on the device.  No synchronisation."""
        _check_seq_crt("skeleton_capsules", "F", seq, crt)
        F = seq.shape[0]
        geom = torch.empty(F * 30, 7, device=self.device, dtype=torch.float64)
        rgb = torch.empty(F * 30, device=self.device, dtype=torch.int32)
        _capi.check(self.lib.gem_skeleton_capsules(_ptr(seq), F, _ptr(crt), int(rgb_joint) & 0xFFFFFF, int(rgb_line) & 0xFFFFFF,
                                                   _ptr(geom), _ptr(rgb), _stream()), self.lib)
        return geom, rgb

    def render_capsules(self, geom, rgb, first, view, out=None, want_ids=False):
        """Image i = the capsules first[i] .. first[i+1] of `geom` [n,7] f64 / `rgb` [n] int32 through `view` (a `_capi.GemView`), as
        PNG scanline streams (gem_render_capsules) -> uint8 [n_images, stride] on the device, `out` when given
        (rows at least the image's bytes, 16-byte aligned, a row stride that is a multiple of 16).  `first`: ascending integers
        (a sequence, or an int32 device tensor).  want_ids: -> (out, ids int32 [n_images,H,W], depth f64 [n_images,H,W]).  Waits for
        the stream once (the library reads `first` back before it launches)."""
        check_tensor(geom, torch.float64, (None, 7), error=TypeError("render_capsules: geom must be a contiguous float64 device tensor [n,7]"))
        check_tensor(rgb, torch.int32, (geom.shape[0],), error=TypeError("render_capsules: rgb must be a contiguous int32 device tensor [n]"))
        if not torch.is_tensor(first):
            first = torch.tensor([int(f) for f in first], dtype=torch.int32).to(self.device)
        check_tensor(first, torch.int32, (None,), at_least=1,
                     error=TypeError("render_capsules: first must be a contiguous int32 device tensor [n_images + 1]"))
        n = first.numel() - 1
        lay = (C.c_int64 * 3)()
        _capi.check(self.lib.gem_render_layout(view.width, view.height, lay), self.lib)
        if out is None:
            out = torch.empty(n, lay[2], device=self.device, dtype=torch.uint8)
        check_tensor(out, torch.uint8, rows=(n, lay[1]),
                     error=ValueError("render_capsules: out must be a uint8 device tensor [%d, >= %d] with contiguous rows" % (n, lay[1])))
        ids = torch.empty(n, view.height, view.width, device=self.device, dtype=torch.int32) if want_ids else None
        depth = torch.empty(n, view.height, view.width, device=self.device, dtype=torch.float64) if want_ids else None
        _capi.check(self.lib.gem_render_capsules(_ptr(geom), _ptr(rgb), geom.shape[0], _ptr(first), n, C.byref(view), _ptr(out),
                                                 out.stride(0), _ptr(ids), _ptr(depth), _stream()), self.lib)
        return (out, ids, depth) if want_ids else out

    def project_sequence(self, seq, cams=None, crt=None):
        """The fisheye image points of `seq` [n,J,3] f64 (contiguous device tensor), moved by `crt` ([13] from `sequence_align`) first
        when given, seen through `cams` [n,4,4] f64 (rigid camera-to-world; None: the points are in the camera's frame) with the
        arithmetic of the reprojection term (gem_project_sequence) -> [n,J,2] f32 on the device, pixels of the
        1280 x 1024 image; a joint on the optical axis gives a pair that is not finite.  No synchronisation."""
        _check_seq_crt("project_sequence", "n", seq, crt)
        n = seq.shape[0]
        if cams is not None:
            check_tensor(cams, torch.float64, error=TypeError("project_sequence: cams must be a contiguous float64 device tensor"))
            check_tensor(cams, torch.float64, (n, 4, 4), error=ValueError("project_sequence: cams must be [%d,4,4], got %s" % (n, tuple(cams.shape))))
        uv = torch.empty(n, N_JOINTS, 2, device=self.device, dtype=torch.float32)
        _capi.check(self.lib.gem_project_sequence(self._h, _ptr(seq), _ptr(crt), _ptr(cams), n, _ptr(uv), _stream()), self.lib)
        return uv

    def render_camera(self, heat, uv, rgb, view, out=None, want_ids=False):
        """The camera's view (gem_render_camera): image i = heat-maps `heat`[i] ([n,H,W,J] f32, or None: white)
        under the skeletons whose image points are `uv` [S,n,J,2] f32 (`project_sequence`), sequence s flat in `rgb`[s] ([S] int32,
        0x00BBGGRR), through `view` (a `_capi.GemCameraView`), as PNG scanline streams -> uint8 [n, stride] on the device, `out` when
        given (rows at least the image's bytes, 16-byte aligned, a row stride that is a multiple of 16).  want_ids: -> (out, ids
        int32 [n,N,N], response f32 [n,N,N]).  No synchronisation."""
        check_tensor(uv, torch.float32, (None, None, N_JOINTS, 2),
                     error=TypeError("render_camera: uv must be a contiguous float32 device tensor [S,n,%d,2]" % N_JOINTS))
        S, n = uv.shape[0], uv.shape[1]
        check_tensor(rgb, torch.int32, (S,), error=TypeError("render_camera: rgb must be a contiguous int32 device tensor [%d]" % S))
        if heat is not None:
            check_tensor(heat, torch.float32, error=TypeError("render_camera: heat must be a contiguous float32 device tensor"))
            check_tensor(heat, torch.float32, (n,) + tuple(self.heat_size) + (N_JOINTS,),
                         error=ValueError("render_camera: heat must be [%d,%d,%d,%d], got %s" % ((n,) + tuple(self.heat_size) + (N_JOINTS, tuple(heat.shape)))))
        lay = (C.c_int64 * 3)()
        _capi.check(self.lib.gem_render_layout(view.size, view.size, lay), self.lib)
        if out is None:
            out = torch.empty(n, lay[2], device=self.device, dtype=torch.uint8)
        check_tensor(out, torch.uint8, rows=(n, lay[1]),
                     error=ValueError("render_camera: out must be a uint8 device tensor [%d, >= %d] with contiguous rows" % (n, lay[1])))
        ids = torch.empty(n, view.size, view.size, device=self.device, dtype=torch.int32) if want_ids else None
        response = torch.empty(n, view.size, view.size, device=self.device, dtype=torch.float32) if want_ids else None
        _capi.check(self.lib.gem_render_camera(self._h, _ptr(heat), _ptr(uv), _ptr(rgb), S, n, C.byref(view), _ptr(out), out.stride(0),
                                               _ptr(ids), _ptr(response), _stream()), self.lib)
        return (out, ids, response) if want_ids else out

    # ------------------------------------------------------------------ JPEG images of rendered frames
    def jpeg_header(self, width, height, quality=90):
        """The 629 bytes in front of an image's entropy data (gem_jpeg_header), as `bytes`.  Needs no GPU work."""
        buf = (C.c_ubyte * 629)()
        if self.lib.gem_jpeg_header(int(width), int(height), int(quality), buf, 629) != 629:
            _capi.check(1, self.lib)
        return bytes(buf)

    def jpeg_bound(self, width, height):
        """The most bytes one width x height image's JPEG file can take (gem_jpeg_bound)."""
        n = self.lib.gem_jpeg_bound(int(width), int(height))
        if n < 0:
            _capi.check(1, self.lib)
        return int(n)

    def jpeg_encode_into(self, scan, width, height, quality, avi, out, offsets, coef=None):
        """gem_jpeg_encode as it is: `scan` uint8 [n, stride] on the device with contiguous rows, `out` a contiguous uint8 device
        tensor (its size is the capacity), `offsets` int64 [n + 1] on the device, `coef` None or int16 [n,3,Hp/8,Wp/8,64].
        Asynchronous; nothing is read back."""
        if not (torch.is_tensor(scan) and scan.is_cuda and scan.dtype == torch.uint8 and scan.dim() == 2 and (scan.shape[0] == 0 or scan.stride(1) == 1)):
            raise TypeError("jpeg_encode: scan must be a uint8 device tensor [n, stride] with contiguous rows")
        n = scan.shape[0]
        check_tensor(out, torch.uint8, error=TypeError("jpeg_encode: out must be a contiguous uint8 device tensor"))
        check_tensor(offsets, torch.int64, numel=n + 1, error=TypeError("jpeg_encode: offsets must be a contiguous int64 device tensor [%d]" % (n + 1)))
        if scan.shape[1] < int(height) * (1 + 3 * int(width)):
            raise ValueError("jpeg_encode: %d x %d pixels are %d scanline bytes, the rows of scan hold %d" %
                             (width, height, int(height) * (1 + 3 * int(width)), scan.shape[1]))
        if coef is not None:
            shape = (n, 3, (int(height) + 7) // 8, (int(width) + 7) // 8, 64)
            check_tensor(coef, torch.int16, shape, error=TypeError("jpeg_encode: coef must be a contiguous int16 device tensor %s" % (shape,)))
        _capi.check(self.lib.gem_jpeg_encode(self._h, _ptr(scan), n, int(width), int(height), scan.stride(0) if n else scan.shape[1], int(quality),
                                             1 if avi else 0, _ptr(out), out.numel(), _ptr(offsets), _ptr(coef), _stream()), self.lib)

    def jpeg_encode(self, scan, width, height, quality=90, avi=False, coef=False, out=None):
        """The images of `scan` -- uint8 [n, stride] on the device, every row the scanline stream `render_capsules` / `render_camera`
        write -- as baseline JPEG (gem_jpeg_encode): (data, offsets[, coefficients]).  Image i is
        data[offsets[i]:offsets[i+1]], a complete JPEG file, or with avi=True the `00dc` chunk of an AVI file; `data` is a uint8
        device tensor of offsets[n] bytes and `offsets` a list of n + 1 integers.  coef=True adds the quantised coefficients, int16
        [n,3,Hp/8,Wp/8,64] in zigzag order, on the device.  `out`: a contiguous uint8 device tensor to encode into when it is large
        enough (default: n times a sixth of the scanline bytes plus the header).  One read-back (the offsets); when the images need more room
        than there was, that much is allocated and the call made once more."""
        n = scan.shape[0]
        want = torch.empty(n, 3, (int(height) + 7) // 8, (int(width) + 7) // 8, 64, device=self.device, dtype=torch.int16) if coef else None
        if out is None:
            out = torch.empty(max(1, n * (1024 + int(height) * (1 + 3 * int(width)) // 6)), device=self.device, dtype=torch.uint8)
        offsets = torch.empty(n + 1, device=self.device, dtype=torch.int64)
        self.jpeg_encode_into(scan, width, height, quality, avi, out, offsets, want)
        at = offsets.tolist()
        if at[n] > out.numel():
            out = torch.empty(at[n], device=self.device, dtype=torch.uint8)
            self.jpeg_encode_into(scan, width, height, quality, avi, out, offsets, want)
        return (out[:at[n]], at, want) if coef else (out[:at[n]], at)

    # ------------------------------------------------------------------ looking at a trained VAE
    PATH_MODES = {"linear": 0, "spherical": 1}
    REPORT_KEYS = ("mu_error", "std_error", "kld", "mpjpe", "max_joint_error")

    def latent_paths(self, za, zb, steps, mode="linear"):
        """`steps` latent points from za to zb for each of P pairs (gem_latent_paths): za, zb [P,D] (or [D]) f32 -> [P,steps,D] f32
        on the device.  The end points are za and zb themselves; mode "linear" is numpy's float32 arithmetic of the reference's
        interpolant.py:126, "spherical" walks the great circle between the two directions.  P is not limited by max_windows.  No
        synchronisation."""
        if mode not in self.PATH_MODES:
            raise ValueError("latent_paths: mode must be one of %s, got %r" % (sorted(self.PATH_MODES), mode))
        a = self._f32(za).reshape(-1, self.D)
        b = self._f32(zb).reshape(-1, self.D)
        if a.shape != b.shape or a.shape[0] < 1:
            raise ValueError("latent_paths: za and zb must be equally shaped [P,%d] with P >= 1, got %s and %s" % (self.D, tuple(a.shape), tuple(b.shape)))
        if int(steps) < 2:
            raise ValueError("latent_paths: a path has at least its two end points (steps >= 2), got %d" % steps)
        out = torch.empty(a.shape[0], int(steps), self.D, device=self.device, dtype=torch.float32)
        _capi.check(self.lib.gem_latent_paths(_ptr(a), _ptr(b), a.shape[0], self.D, int(steps), self.PATH_MODES[mode], _ptr(out), _stream()),
                    self.lib)
        return out

    def latent_report(self, mu, logvar, x=None, rec=None, cols=None, count=None, out=None):
        """What a batch of encoded (and reconstructed) windows says about the VAE (gem_latent_report): mu, logvar [B,D] f32, x and
        rec [B,T,45] f32 or both None -> [B,5] f64 on the device in the order of REPORT_KEYS (`out` when given: a contiguous f64
        device tensor [B,5]; the last two NaN without x / rec).  cols [3,D] f64 and count [1] i64 are device accumulators the
        caller zeroes once: every call adds the batch's sum mu_d, sum mu_d^2, sum exp(logvar_d) and B.  B is not limited by
        max_windows.  No synchronisation."""
        if (x is None) != (rec is None):
            raise ValueError("latent_report: x and rec come together")
        check_tensors("latent_report", (mu, torch.float32, None), (logvar, torch.float32, None), (x, torch.float32, None), (rec, torch.float32, None),
                      (cols, torch.float64, None), (count, torch.int64, None), (out, torch.float64, None))
        B = mu.shape[0]
        if mu.dim() != 2 or tuple(mu.shape) != (B, self.D) or tuple(logvar.shape) != (B, self.D) or B < 1:
            raise ValueError("latent_report: mu and logvar must be [B,%d] with B >= 1, got %s and %s" % (self.D, tuple(mu.shape), tuple(logvar.shape)))
        n_coords = self.T * N_JOINTS * 3
        if x is not None and not (x.numel() == B * n_coords and rec.numel() == B * n_coords):
            raise ValueError("latent_report: x and rec must hold %d windows of %d x %d x 3 values" % (B, self.T, N_JOINTS))
        if cols is not None and tuple(cols.shape) != (3, self.D):
            raise ValueError("latent_report: cols must be [3,%d]" % self.D)
        if count is not None and count.numel() != 1:
            raise ValueError("latent_report: count must hold one int64")
        if out is None:
            out = torch.empty(B, 5, device=self.device, dtype=torch.float64)
        if tuple(out.shape) != (B, 5):
            raise ValueError("latent_report: out must be [%d,5]" % B)
        _capi.check(self.lib.gem_latent_report(_ptr(mu), _ptr(logvar), _ptr(x), _ptr(rec), B, self.D, n_coords, N_JOINTS, _ptr(out),
                                               _ptr(cols), _ptr(count), _stream()), self.lib)
        return out

    # ------------------------------------------------------------------ live mode
    def live_buffers(self):
        """The device memory of one live session (gem_live_buffers): the frame rings and the zeroed state block, as a dict of
        tensors plus "c", the struct the library is handed (it holds their addresses: keep the dict alive)."""
        H, W = self.heat_size
        t = {"ring_pose": torch.zeros(_capi.LIVE_RING, N_JOINTS, 3, device=self.device, dtype=torch.float32),
             "ring_cams": torch.zeros(_capi.LIVE_RING, 4, 4, device=self.device, dtype=torch.float64),
             "ring_times": torch.zeros(_capi.LIVE_RING, device=self.device, dtype=torch.float64),
             "ring_heat": torch.zeros(_capi.LIVE_RING, H, W, N_JOINTS, device=self.device, dtype=torch.float32),
             "state": torch.zeros(_capi.LIVE_STATE_DOUBLES, device=self.device, dtype=torch.float64)}
        t["c"] = _capi.GemLiveBuffers(*[t[k].data_ptr() for k, _ in _capi.GemLiveBuffers._fields_])
        return t

    def live_push(self, bufs, first_frame, oldest_needed, heat, pose, cams, times):
        """k <= 8 frames into the rings of `bufs` (`live_buffers`) as the frames first_frame .. first_frame + k - 1 (gem_live_push):
        heat [k,H,W,15] f32, pose [k,15,3] f32, cams [k,4,4] f64, times [k] f64, contiguous device tensors.  oldest_needed: the
        oldest frame a window still to come reads.  No synchronisation."""
        k = int(times.shape[0]) if torch.is_tensor(times) and times.dim() == 1 else -1
        check_tensors("live_push", (heat, torch.float32, (k,) + self.heat_size + (N_JOINTS,)), (pose, torch.float32, (k, N_JOINTS, 3)),
                      (cams, torch.float64, (k, 4, 4)), (times, torch.float64, (k,)))
        _capi.check(self.lib.gem_live_push(self._h, C.byref(bufs["c"]), int(first_frame), k, int(oldest_needed), _ptr(heat), _ptr(pose),
                                           _ptr(cams), _ptr(times), _stream()), self.lib)

    def live_window(self, bufs, window, n_pushed, win_pose, win_cams, win_heat, mean_bone, bone_fixed=None):
        """The frames [8 window, 8 window + 10) from the rings into the window buffers win_pose [10,15,3] f32, win_cams [10,4,4] f64,
        win_heat [10,H,W,15] f32, and the call's mean bone lengths into mean_bone [1,15] f32: `bone_fixed` [15] f32 when given, else
        the running mean over the frames pushed so far (gem_live_window).  No synchronisation."""
        check_tensors("live_window", (win_pose, torch.float32, (self.T, N_JOINTS, 3)), (win_cams, torch.float64, (self.T, 4, 4)),
                      (win_heat, torch.float32, (self.T,) + self.heat_size + (N_JOINTS,)), (mean_bone, torch.float32, (1, N_JOINTS)),
                      (bone_fixed, torch.float32, (N_JOINTS,)))
        _capi.check(self.lib.gem_live_window(self._h, C.byref(bufs["c"]), int(window), int(n_pushed), _ptr(bone_fixed), _ptr(win_pose),
                                             _ptr(win_cams), _ptr(win_heat), _ptr(mean_bone), _stream()), self.lib)

    def live_emit(self, bufs, window, out, glob=None, win_pose=None, win_cams=None, final=False, one_euro=None):
        """The window's result `glob` [1,10,15,3] f64 (optimize_windows on the window buffers) -> out [2,8,15,3] f64: the 8 frames
        the window makes final, optimised (out[0]; merged with the two held frames, One-Euro filtered when `one_euro` = (min_cutoff,
        beta, d_cutoff)) and estimated (out[1]); the window's last two frames are held (gem_live_emit).  final=True: the two held
        frames into out[:, :2] instead.  No synchronisation."""
        check_tensors("live_emit", (out, torch.float64, (2, _capi.LIVE_STRIDE, N_JOINTS, 3)), (glob, torch.float64, (1, self.T, N_JOINTS, 3)),
                      (win_pose, torch.float32, (self.T, N_JOINTS, 3)), (win_cams, torch.float64, (self.T, 4, 4)))
        euro = (C.c_double * 3)(*[float(v) for v in one_euro]) if one_euro is not None else None
        _capi.check(self.lib.gem_live_emit(self._h, C.byref(bufs["c"]), int(window), 1 if final else 0, _ptr(glob), _ptr(win_pose),
                                           _ptr(win_cams), euro, _ptr(out), _stream()), self.lib)
        return out

    def live_dense_state(self):
        """The second block of a dense live session (include/gem_live_dense.h): the per-frame sums and counts, the estimated frames
        still held and the `now` stream's filter state, zeroed."""
        return torch.zeros(_capi.LIVE_DENSE_DOUBLES, device=self.device, dtype=torch.float64)

    def live_window_at(self, bufs, first_frame, n_pushed, win_pose, win_cams, win_heat, mean_bone, bone_fixed=None):
        """`live_window` for the frames [first_frame, first_frame + 10) (gem_live_window_at).  No synchronisation."""
        check_tensors("live_window_at", (win_pose, torch.float32, (self.T, N_JOINTS, 3)), (win_cams, torch.float64, (self.T, 4, 4)),
                      (win_heat, torch.float32, (self.T,) + self.heat_size + (N_JOINTS,)), (mean_bone, torch.float32, (1, N_JOINTS)),
                      (bone_fixed, torch.float32, (N_JOINTS,)))
        _capi.check(self.lib.gem_live_window_at(self._h, C.byref(bufs["c"]), int(first_frame), int(n_pushed), _ptr(bone_fixed), _ptr(win_pose),
                                                _ptr(win_cams), _ptr(win_heat), _ptr(mean_bone), _stream()), self.lib)

    def live_emit_dense(self, bufs, dense_state, stride, window, out, glob=None, win_pose=None, win_cams=None, final=False, one_euro=None):
        """The result `glob` [1,10,15,3] f64 of window `window` at `stride` (1..8) -> out [3,10,15,3] f64 (gem_live_emit_dense):
        out[0, :stride] the frames no later window covers, each the mean of the windows that covered it (oldest first, never
        filtered); out[1, :stride] their estimated frames; out[2] the `now` frames -- all 10 of window 0, else the window's last
        `stride` -- unaveraged, One-Euro filtered when `one_euro` = (min_cutoff, beta, d_cutoff).  final=True (`window` = the number of
        windows emitted): the 10 - stride frames still held into out[0] and out[1] instead.  `dense_state`: `live_dense_state()`.
        No synchronisation."""
        check_tensors("live_emit_dense", (dense_state, torch.float64, (_capi.LIVE_DENSE_DOUBLES,)), (out, torch.float64, (3, self.T, N_JOINTS, 3)),
                      (glob, torch.float64, (1, self.T, N_JOINTS, 3)), (win_pose, torch.float32, (self.T, N_JOINTS, 3)),
                      (win_cams, torch.float64, (self.T, 4, 4)))
        if dense_state is None:
            raise TypeError("live_emit_dense wants the session's dense state block")
        euro = (C.c_double * 3)(*[float(v) for v in one_euro]) if one_euro is not None else None
        _capi.check(self.lib.gem_live_emit_dense(self._h, C.byref(bufs["c"]), _ptr(dense_state), int(stride), int(window), 1 if final else 0,
                                                 _ptr(glob), _ptr(win_pose), _ptr(win_cams), euro, _ptr(out), _stream()), self.lib)
        return out

    def merge_dense(self, windows, n_chunks, stride):
        """Every frame the mean of all windows that cover it, per chunk (gem_merge_dense; `sequence.merge_dense` on the device):
        windows [n_chunks*wpc,T,15,3] at `stride` (1..T) frames from one another -> [n_chunks, (wpc-1)*stride + T, 15, 3] f64.  Overlaps
        above T / 2, which `merge_windows` does not serve, included.  No synchronisation."""
        w = self._f64(windows).reshape(-1, self.T, N_JOINTS, 3)
        if n_chunks < 1 or w.shape[0] == 0 or w.shape[0] % n_chunks:
            raise ValueError("merge_dense: %d windows do not split into %d chunks" % (w.shape[0], n_chunks))
        if not 1 <= int(stride) <= self.T:
            raise ValueError("merge_dense: the stride is between 1 and %d frames, got %r" % (self.T, stride))
        wpc = w.shape[0] // n_chunks
        out = torch.empty(n_chunks, (wpc - 1) * int(stride) + self.T, N_JOINTS, 3, device=self.device, dtype=torch.float64)
        _capi.check(self.lib.gem_merge_dense(_ptr(w), n_chunks, wpc, self.T, N_JOINTS * 3, int(stride), _ptr(out), _stream()), self.lib)
        return out

    def merge_cover(self, windows, starts, smooth=False, want_spread=False):
        """Every frame the mean of all windows that cover it, for windows that are not equally spaced (gem_merge_cover;
        `sequence.merge_cover` on the device): windows [B,T,J,3] at `starts` [B] -> (merged [N,J,3] f64, its
        Gaussian-smoothed copy with `smooth` else None, count [N] i32, spread [N] f64 with `want_spread` else None), N = starts[-1] + T,
        device tensors.  `starts`: host integers, checked with `sequence.check_cover` and uploaded, or an int32 device tensor the caller
        vouches for (its last entry is read back for N).  No other synchronisation."""
        from .sequence import check_cover
        w = self._f64(windows)
        if w.dim() != 4 or w.shape[3] != 3 or not 1 <= w.shape[2] <= 16 or w.shape[1] < 1 or w.shape[0] < 1:
            raise ValueError("merge_cover: windows must be [B,T,J,3] with J <= 16, got %s" % (tuple(w.shape),))
        B, T, J = w.shape[0], w.shape[1], w.shape[2]
        if torch.is_tensor(starts) and starts.is_cuda:
            if starts.dtype != torch.int32 or not starts.is_contiguous() or tuple(starts.shape) != (B,):
                raise TypeError("merge_cover: device starts must be a contiguous int32 tensor [%d]" % B)
            s_d, n = starts, int(starts[-1].item()) + T
        else:
            s = check_cover(starts.cpu().numpy() if torch.is_tensor(starts) else starts, T)
            if len(s) != B:
                raise ValueError("merge_cover: %d starts for %d windows" % (len(s), B))
            if int(s[-1]) + T > 2 ** 31 - 1:
                raise ValueError("merge_cover: window starts are 32-bit frame numbers")
            s_d, n = torch.from_numpy(s.astype(np.int32)).to(self.device), int(s[-1]) + T
        merged = torch.empty(n, J, 3, device=self.device, dtype=torch.float64)
        smoothed = torch.empty_like(merged) if smooth else None
        count = torch.empty(n, device=self.device, dtype=torch.int32)
        spread = torch.empty(n, device=self.device, dtype=torch.float64) if want_spread else None
        _capi.check(self.lib.gem_merge_cover(_ptr(w), _ptr(s_d), B, T, J, n, _ptr(merged), _ptr(smoothed), _ptr(count), _ptr(spread), _stream()),
                    self.lib)
        return merged, smoothed, count, spread

    def one_euro_filter(self, seq, times, n_chunks, params):
        """The reference's utils/one_euro_filter.py over `n_chunks` equally long sequences laid end to end (gem_one_euro): seq
        [n_chunks*F,15,3] f64 (any trailing shape), times [n_chunks*F] f64, params (min_cutoff, beta, d_cutoff) -> a device tensor
        of seq's shape; every chunk starts with fresh state.  No synchronisation."""
        s, t = self._f64(seq), self._f64(times).reshape(-1)
        total = t.shape[0]
        if n_chunks < 1 or total % n_chunks or s.dim() < 2 or s.shape[0] != total:
            raise ValueError("one_euro_filter: %d timestamps for a sequence of shape %s in %d chunks" % (total, tuple(s.shape), n_chunks))
        if len(params) != 3:
            raise ValueError("one_euro_filter: params are (min_cutoff, beta, d_cutoff)")
        out = torch.empty_like(s)
        if total == 0:
            return out
        euro = (C.c_double * 3)(*[float(v) for v in params])
        _capi.check(self.lib.gem_one_euro(_ptr(s), _ptr(t), int(n_chunks), total // n_chunks, s.numel() // total, euro, _ptr(out), _stream()),
                    self.lib)
        return out

    def calculate_errors(self, est, mid, opt, gt):
        """Same keys and definitions as the reference's calculate_errors (calculate_errors.py:114-179)."""
        from collections import OrderedDict
        v = self.calculate_errors_device(est, mid, opt, gt).cpu().numpy()
        r = OrderedDict((k, float(v[i])) for i, k in enumerate(self.ERROR_KEYS))
        r["joints_error"] = v[17:].copy()
        return r

    # ------------------------------------------------------------------ input lifting
    def lift_skeleton(self, heat, depth, upscale=16, pad_x=128, pad_y=0, want_f64=True):
        """heat [F,H,W,15] f32 + depth [F,15] -> estimated_local_skeleton [F,15,3] (f64 like the reference's pickle,
        and f32 for optimize_windows): heat-map argmax + fisheye un-projection (utils/skeleton.py:32-45,176-204)."""
        heat_t = self._f32(heat)
        if heat_t.dim() != 4 or tuple(heat_t.shape[1:]) != (self.heat_size[0], self.heat_size[1], N_JOINTS):
            raise ValueError("lift_skeleton wants heat-maps [F,%d,%d,%d]" % (self.heat_size[0], self.heat_size[1], N_JOINTS))
        F = heat_t.shape[0]
        dep = self._f64(depth).reshape(F, N_JOINTS)
        poly = np.ascontiguousarray(self.camera.poly_c2w, dtype=np.float64)
        o64 = torch.empty(F, N_JOINTS, 3, device=self.device, dtype=torch.float64) if want_f64 else None
        o32 = torch.empty(F, N_JOINTS, 3, device=self.device, dtype=torch.float32)
        _capi.check(self.lib.gem_lift_skeleton(self._h, _ptr(heat_t), _ptr(dep), F, poly.ctypes.data_as(C.POINTER(C.c_double)),
                                               len(poly), upscale, pad_x, pad_y, _ptr(o64), _ptr(o32), _stream()), self.lib)
        return o64, o32

    # ------------------------------------------------------------------ 2-D joint detections
    def _keypoints(self, what, kp):
        """[F,15,2|3] detections (u, v[, confidence]) -> a contiguous [F,15,3] f64 device tensor; without a third column every
        confidence is 1."""
        t = self._f64(kp)
        if t.dim() != 3 or t.shape[1] != N_JOINTS or t.shape[2] not in (2, 3):
            raise ValueError("%s wants detections [F,%d,2] or [F,%d,3], got %s" % (what, N_JOINTS, N_JOINTS, tuple(t.shape)))
        if t.shape[2] == 2:
            t = torch.cat([t, torch.ones_like(t[..., :1])], dim=2).contiguous()
        return t

    def keypoint_heatmaps(self, kp, sigma=1.5, out=None):
        """kp [F,15,2|3] (u, v in pixels of the fisheye image[, confidence]) -> heat [F,H,W,15] f32 at the engine's `heat_size`: unit-peak
        Gaussians times the clamped confidence, centred where the reprojection term samples (u, v); a blank map for an unusable
        detection (gem_keypoint_heatmaps).  `out`: a contiguous float32 device tensor of that shape to write into.  No synchronisation."""
        t = self._keypoints("keypoint_heatmaps", kp)
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma > 0):
            raise ValueError("keypoint_heatmaps: sigma must be a positive number, got %r" % sigma)
        F, (H, W) = t.shape[0], self.heat_size
        if out is None:
            out = torch.empty(F, H, W, N_JOINTS, device=self.device, dtype=torch.float32)
        check_tensors("keypoint_heatmaps", (out, torch.float32, (F, H, W, N_JOINTS)))
        _capi.check(self.lib.gem_keypoint_heatmaps(_ptr(t), F, N_JOINTS, H, W, sigma, _ptr(out), _stream()), self.lib)
        return out

    def lift_keypoints(self, kp, depth, prev=None, want_f64=True):
        """kp [F,15,2|3] + depth [F,15] -> (o64 [F,15,3] f64 or None, o32 [F,15,3] f32, valid [F,15] u8): camera2world at the sub-pixel
        detection (gem_lift_keypoints).  prev None: an unusable joint is zeros (`fill_missing` replaces it).  prev [15,3] f64, a
        contiguous device tensor: frames in order, an unusable joint takes prev's value, every usable one updates it, in place."""
        t = self._keypoints("lift_keypoints", kp)
        F = t.shape[0]
        dep = self._f64(depth)
        if dep.numel() != F * N_JOINTS:
            raise ValueError("lift_keypoints wants depth [F,%d] for these %d frames, got %s" % (N_JOINTS, F, tuple(dep.shape)))
        check_tensors("lift_keypoints", (prev, torch.float64, (N_JOINTS, 3)))
        poly = np.ascontiguousarray(self.camera.poly_c2w, dtype=np.float64)
        o64 = torch.empty(F, N_JOINTS, 3, device=self.device, dtype=torch.float64) if want_f64 else None
        o32 = torch.empty(F, N_JOINTS, 3, device=self.device, dtype=torch.float32)
        valid = torch.empty(F, N_JOINTS, device=self.device, dtype=torch.uint8)
        _capi.check(self.lib.gem_lift_keypoints(self._h, _ptr(t), _ptr(dep), F, poly.ctypes.data_as(C.POINTER(C.c_double)), len(poly),
                                                _ptr(prev), _ptr(o64), _ptr(o32), _ptr(valid), _stream()), self.lib)
        return o64, o32, valid

    def fill_missing(self, seq, valid, n_chunks):
        """In place on seq [n_chunks*F,15,3] f64 with valid [n_chunks*F,15] u8 (contiguous device tensors): per chunk and joint, frames
        with valid 0 become the linear interpolation in time between their valid neighbours, the nearest valid value at the chunk's
        ends (gem_fill_missing).  A joint with no valid frame in a chunk stays as it is.  -> seq.  No synchronisation."""
        total = int(seq.shape[0]) if torch.is_tensor(seq) and seq.dim() == 3 else -1
        if n_chunks < 1 or total < 0 or total % n_chunks:
            raise ValueError("fill_missing: a sequence [n,%d,3] of %d equal chunks is wanted" % (N_JOINTS, n_chunks))
        check_tensors("fill_missing", (seq, torch.float64, (total, N_JOINTS, 3)), (valid, torch.uint8, (total, N_JOINTS)))
        _capi.check(self.lib.gem_fill_missing(_ptr(seq), _ptr(valid), int(n_chunks), total // n_chunks, N_JOINTS, _stream()), self.lib)
        return seq

    def bone_depths(self, kp, bones=None, rest=None, neck_depth=None, iters=None, out=None, opts=None):
        """kp [F,15,2|3] -> (depth [F,15] f64, solved [F,15] u8, rms [F] f64), device tensors: per frame the depths along the
        detections' rays that meet the bone lengths, the neck's anchor and the prior (gem_bone_depths).
        `bones`, `rest`, `neck_depth`, `iters`: `bone_depth.options`; `opts`: its result, in their place.  An unsolved joint (solved 0)
        keeps its prior depth.  rms: the frame's RMS bone-length residual in metres.  `out`: (depth, solved, rms) contiguous device
        tensors of those shapes to write into (None entries are allocated).  No synchronisation."""
        from . import bone_depth
        if opts is None:
            opts = bone_depth.options(bones, rest, neck_depth, iters)
        t = self._keypoints("bone_depths", kp)
        F = t.shape[0]
        depth, solved, rms = out if out is not None else (None, None, None)
        check_tensors("bone_depths", (depth, torch.float64, (F, N_JOINTS)), (solved, torch.uint8, (F, N_JOINTS)), (rms, torch.float64, (F,)))
        depth = torch.empty(F, N_JOINTS, device=self.device, dtype=torch.float64) if depth is None else depth
        solved = torch.empty(F, N_JOINTS, device=self.device, dtype=torch.uint8) if solved is None else solved
        rms = torch.empty(F, device=self.device, dtype=torch.float64) if rms is None else rms
        o = _capi.GemBoneDepthOpts(neck_depth=opts["neck_depth"], w_n=opts["w_n"], w_m=opts["w_m"], iters=opts["iters"], reserved=0)
        for j in range(N_JOINTS):
            o.bone[j], o.dbar[j] = float(opts["L"][j]), float(opts["dbar"][j])
        poly = np.ascontiguousarray(self.camera.poly_c2w, dtype=np.float64)
        _capi.check(self.lib.gem_bone_depths(self._h, _ptr(t), F, poly.ctypes.data_as(C.POINTER(C.c_double)), len(poly), C.byref(o),
                                             _ptr(depth), _ptr(solved), _ptr(rms), _stream()), self.lib)
        return depth, solved, rms

    def heatmap_peaks(self, heat, min_peak=0.0, out=None, upscale=16, pad_x=128, pad_y=0):
        """heat [F,H,W,15] f32 at the engine's `heat_size` -> (kp [F,15,3] f64, arg [F,15] int32), device tensors: per joint the
        map's peak as a detection (u, v, confidence) -- the integer maximum refined by a Gaussian-windowed mean shift, in the pixels of
        the fisheye image, confidence = min(peak, 1) -- and the flat index of the integer maximum (gem_heatmap_peaks, DESIGN.md section
        6r).  A joint whose peak is NaN, not positive or below `min_peak` is (0, 0, 0): an unusable detection.  `out`: (kp, arg)
        contiguous device tensors of those shapes to write into (a None entry is allocated).  No synchronisation."""
        heat_t = self._f32(heat)
        if heat_t.dim() != 4 or tuple(heat_t.shape[1:]) != (self.heat_size[0], self.heat_size[1], N_JOINTS):
            raise ValueError("heatmap_peaks wants heat-maps [F,%d,%d,%d], got %s" % (self.heat_size[0], self.heat_size[1], N_JOINTS, tuple(heat_t.shape)))
        min_peak = float(min_peak)
        if not (np.isfinite(min_peak) and min_peak >= 0):
            raise ValueError("heatmap_peaks: min_peak must be a finite number >= 0, got %r" % min_peak)
        F = heat_t.shape[0]
        kp, arg = out if out is not None else (None, None)
        check_tensors("heatmap_peaks", (kp, torch.float64, (F, N_JOINTS, 3)), (arg, torch.int32, (F, N_JOINTS)))
        kp = torch.empty(F, N_JOINTS, 3, device=self.device, dtype=torch.float64) if kp is None else kp
        arg = torch.empty(F, N_JOINTS, device=self.device, dtype=torch.int32) if arg is None else arg
        _capi.check(self.lib.gem_heatmap_peaks(self._h, _ptr(heat_t), F, int(upscale), int(pad_x), int(pad_y), min_peak, _ptr(kp), _ptr(arg),
                                               _stream()), self.lib)
        return kp, arg

    # ------------------------------------------------------------------ profiling hook (bench.py)
    def profile_enable(self, on):
        _capi.check(self.lib.gem_profile_enable(self._h, 1 if on else 0), self.lib)

    def profile_kernels(self, family):
        """Names (as rocprofv3 prints them) of the kernels launched for `family` while profiling was on, since the last call."""
        buf = C.create_string_buffer(2048)
        _capi.check(self.lib.gem_profile_kernels(self._h, family, buf, len(buf)), self.lib)
        return buf.value.decode()

    def profile_read(self, family):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        _capi.check(self.lib.gem_profile_read(self._h, family, C.byref(ms), C.byref(n), C.byref(fl)), self.lib)
        return ms.value, n.value, fl.value


def stats_to_numpy(stats):
    """[n,4] int32 tensor (n_iter, func_evals, final_loss bits, status) -> structured numpy.

    `status` is a bit field (gem_window_stats): bit 0 = the window's L-BFGS finished, bit 1 = a closure value was NaN (a joint
    on the optical axis: the reference raises "norm is zero!").  `finished` / `degenerate` are those two bits as booleans;
    `status == 1` therefore reads "finished and not degenerate"."""
    a = stats.cpu().numpy()
    out = np.zeros(a.shape[0], dtype=[("n_iter", "i4"), ("func_evals", "i4"), ("final_loss", "f4"), ("status", "i4"),
                                      ("finished", "?"), ("degenerate", "?")])
    out["n_iter"], out["func_evals"], out["status"] = a[:, 0], a[:, 1], a[:, 3]
    out["final_loss"] = a[:, 2].copy().view(np.float32)
    out["finished"], out["degenerate"] = (a[:, 3] & 1) != 0, (a[:, 3] & 2) != 0
    return out


def raise_if_degenerate(stats):
    """The reference's `Exception("norm is zero!")` (FishEyeCalibrated.py:124-127) for users of the engine's own calls: pass the
    stats tensor (or its stats_to_numpy) of optimize_stage / optimize_windows.  Synchronises on the stats."""
    st = stats if isinstance(stats, np.ndarray) else stats_to_numpy(stats)
    if st["degenerate"].any() or not np.isfinite(st["final_loss"]).all():
        raise Exception("norm is zero!")
