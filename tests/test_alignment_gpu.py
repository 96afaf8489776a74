"""The similarity alignment of csrc/umeyama_device.h on the device, on the point sets and sequences of tests/umeyama_twin.py where
its special branches run (the rank threshold, the completion of U for rank 2, 1 and 0, the tie-break of `kmin`, the reflection with
equal or zero singular values): gem_sequence_align against LAPACK (`errors.umeyama`) and against the twin, the error report
(`engine.calculate_errors`, per frame and per sequence) and its batched form against the host mirror `errors.calculate_errors`, the
same bytes on every call, and the bits of a rank-3 input unchanged by the completion by rank.

Allowances: umeyama_twin.RTOL = 1e-12 for (c, R, t), the aligned points, properness and the squared residual (see
`umeyama_twin.deviations` for how each figure is formed and tests/test_alignment_cpu.py for the three cases compared on what is
unique in them); rtol = 1e-9, atol = 1e-12 for the report's keys as in tests/test_hip_post.py.

Measured on an MI355X, largest per family, device against LAPACK (against the twin: at most 1.1e-15 in every figure; `pytest -s`
prints both tables):
    thickness                  c 1.2e-15  R 1.0e-15  t 1.4e-15  aligned 8.2e-16  orthonormal 5.6e-16  det 7.8e-16
    thickness mirrored         c 1.1e-15  R 1.1e-15  t 1.7e-15  aligned 7.4e-16  orthonormal 8.9e-16  det 1.1e-15
    equal singular values      c 0        R 2.6e-15  t 1.5e-15  aligned 1.4e-15  orthonormal 4.4e-16  det 2.2e-16
    isotropic mirrored         c 2.2e-16  residual 4.4e-16                       orthonormal 3.3e-16  det 4.4e-16
    offset                     c 2.2e-16  R 5.6e-16  t 2.8e-16  aligned 2.8e-16  orthonormal 4.4e-16  det 0
    scale                      c 4.4e-16  R 8.9e-16  t 3.6e-16  aligned 2.9e-16  orthonormal 4.4e-16  det 4.4e-16
    identity                   c 2.2e-16  R 5.0e-16  t 3.7e-16  aligned 2.7e-16  orthonormal 4.4e-16  det 2.2e-16
    180 degrees                c 0        R 3.3e-16  t 7.4e-17  aligned 3.8e-16  orthonormal 2.2e-16  det 2.2e-16
    rank 1                     c 3.3e-16  R on the line 3.3e-16  aligned 2.4e-16  residual 0  orthonormal 7.8e-16  det 1.0e-15
    N = 3 .. 1035              c 1.1e-15  R 6.7e-16  t 1.7e-15  aligned 1.2e-15  orthonormal 4.4e-16  det 6.7e-16
    the report against errors.calculate_errors, largest relative difference of the 17 + 15 numbers: F = 24 1.6e-15, F = 11 2.9e-15,
    F = 33 1.4e-15, the collinear sequence of the batched call 3.3e-15
No family needs more than a hundredth of its allowance.  Every test takes under 0.03 s after the engine is up.

Mutations of the device code, each in a library of its own on the MI355X, none kept:
    `kmin` the largest singular value    red: the mirrored thickness members 1 .. 1e-6 (c off by a factor 1.6, R by 1.7) and the three
                                         report tests (some squashed frames need the reflection); "isotropic mirrored" stays green, as
                                         it must: with three equal values any of them may carry the sign
    the reflection dropped               red: the same, and "isotropic mirrored" (det R = -1, residual off by a factor 2)
    the rank threshold 1e-14 -> 1e-6     red: thickness 1e-4 and 1e-5, plain and mirrored (c off by 1e-9 and 1e-11: the third singular
                                         value is dropped from the sum), and the three report tests; thickness 1e-6 stays green: its
                                         third singular value is 1.2e-13 of the first, so dropping it moves c by less than the allowance
    the completion as it was before      red: both rank-1 cases (source collinear: |R R^T - I| = 0.43, |det R - 1| = 0.23, aligned points 4.5 cm
    svd3 completed U by rank             off; target collinear: |R R^T - I| = 1.7e-4), the constant target, the report at F = 11 and 33
                                         and the batched report (row 1 is not the bytes of its own single call); the report at F = 24
                                         stayed green in that build: what the unwritten column holds is whatever the registers held
A completion of the other handedness cannot be told from the kept one: det U = -1 sets d[kmin] = -1 on a singular value that is
zero, which turns the basis back (tests/test_alignment_cpu.py keeps that on record with the twin)."""
import numpy as np
import pytest

import umeyama_twin as T
from globalegomocap_amd.camera import FisheyeCamera, DEFAULT_CALIBRATION
from globalegomocap_amd.errors import calculate_errors
from helpers import TINY

pytestmark = pytest.mark.gpu

NAMES = list(T.cases())
WORST_LAPACK, WORST_TWIN = T.Worst(), T.Worst()
REPORT_TOL = dict(rtol=1e-9, atol=1e-12)


@pytest.fixture(scope="module")
def engine():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd.engine import WindowEngine
    return WindowEngine(TINY, FisheyeCamera.from_json(DEFAULT_CALIBRATION), max_windows=8)


@pytest.fixture(scope="module")
def twin13():
    """The twin's 13 numbers of every case: computed once."""
    out = {}
    for name, (P, Q, _) in T.cases().items():
        out[name] = T.crt13(*T.umeyama(P, Q))
        out[name].setflags(write=False)
    return out


def _align(engine, P, Q):
    """gem_sequence_align twice -> the 13 numbers, after asserting that the two calls gave the same bytes."""
    import torch
    p, q = torch.from_numpy(np.array(P)).to(engine.device), torch.from_numpy(np.array(Q)).to(engine.device)
    a, b = engine.sequence_align(p, q).cpu().numpy(), engine.sequence_align(p, q).cpu().numpy()
    assert a.tobytes() == b.tobytes(), (a, b)
    return a


@pytest.mark.parametrize("name", NAMES)
def test_sequence_align_against_lapack_and_the_twin(engine, twin13, name):
    P, Q, _ = T.cases()[name]
    got = _align(engine, P, Q)
    WORST_LAPACK.see(name, T.check(name, got, T.reference(name), "device against LAPACK"))
    WORST_TWIN.see(name, T.check(name, got, twin13[name], "device against the twin"))


def test_report_of_the_largest_deviations(engine, twin13, capsys):
    """(after the cases above: prints what the docstring records)"""
    for name in NAMES:
        P, Q, _ = T.cases()[name]
        got = _align(engine, P, Q)
        WORST_LAPACK.see(name, T.deviations(name, got, T.reference(name)))
        WORST_TWIN.see(name, T.deviations(name, got, twin13[name]))
    with capsys.disabled():
        print("\n" + "\n".join(WORST_LAPACK.lines("device against LAPACK") + WORST_TWIN.lines("device against the twin")))


def test_a_constant_target_is_rank_zero(engine):
    """cov = 0 exactly (a dyadic constant): U = I, so c = 0, R the identity and t the target."""
    P = np.array(T.cases()["N = 15"][0])
    Q = np.tile(np.array([0.5, -1.25, 2.0]), (15, 1))
    got = _align(engine, P, Q)
    assert got[0] == 0.0 and np.array_equal(got[1:10].reshape(3, 3), np.eye(3)) and np.array_equal(got[10:], Q[0]), got
    assert np.array_equal(got, T.crt13(*T.umeyama(P, Q)))


def test_rank_three_bits_are_those_of_the_code_before_the_completion_by_rank(engine, golden):
    """An existing case, tests/test_hip_post.py's golden run: the report and the alignment of its sequences, bit for bit what the
    library gave before svd3 completed U by rank (tests/golden/alignment_bits.npz, recorded from that build on an MI355X)."""
    import torch
    g, want = golden("pipeline_tiny"), golden("alignment_bits")
    est, mid, opt, gt = (np.ascontiguousarray(g[k]) for k in ("est_smooth", "mid_local_smooth", "opt_smooth", "gt_smooth"))
    report = engine.calculate_errors_device(est, mid, opt, gt).cpu().numpy()
    crt = engine.sequence_align(torch.from_numpy(est).to(engine.device), torch.from_numpy(gt).to(engine.device)).cpu().numpy()
    assert report.tobytes() == want["report"].tobytes(), np.abs(report - want["report"]).max()
    assert crt.tobytes() == want["crt"].tobytes(), np.abs(crt - want["crt"]).max()


# ------------------------------------------------------------------------------------------------ the error report
_HOST = {}


def _host_report(key, seqs):
    """errors.calculate_errors of a set of sequences: computed once."""
    if key not in _HOST:
        _HOST[key] = calculate_errors(*seqs)
    return _HOST[key]


def _compare_report(got, ref, what):
    """got: the device's 17 + 15 numbers; ref: the host mirror's dict -> the largest relative difference."""
    from globalegomocap_amd.engine import WindowEngine
    assert list(ref.keys()) == list(WindowEngine.ERROR_KEYS) + ["joints_error"] and got.shape == (32,) and np.isfinite(got).all(), got
    worst = 0.0
    for i, k in enumerate(WindowEngine.ERROR_KEYS):
        worst = max(worst, abs(got[i] / ref[k] - 1.0))
        np.testing.assert_allclose(got[i], ref[k], err_msg="%s: %s" % (what, k), **REPORT_TOL)
    worst = max(worst, float(np.abs(got[17:] / ref["joints_error"] - 1.0).max()))
    np.testing.assert_allclose(got[17:], ref["joints_error"], err_msg="%s: joints_error" % what, **REPORT_TOL)
    return worst


def _report(engine, seqs):
    """calculate_errors_device of read-only host sequences (copied: torch wants writable arrays) -> 17 + 15 numbers."""
    return engine.calculate_errors_device(*map(np.array, seqs)).cpu().numpy()


@pytest.mark.parametrize("F", [24, 11, 33])
def test_error_report_on_squashed_frames(engine, F, capsys):
    """Three frames of est / mid / opt per thickness of the sweep, one squashed to a plane and two towards a line, which they reach
    at thickness 0 (F = 24: every thickness; F = 11 and 33 start from thickness 0 and their 6 F tasks end inside a 64-thread
    workgroup), gt generic: all 18 keys against the host mirror, and the same bytes from two calls."""
    seqs, squash = T.sequences(F, 20 + F, descending=F == 24)
    assert sum(map(T.is_line, squash)) >= 2 and ("z", 0.0) in squash and (6 * F) % 64 != 0
    a = _report(engine, seqs)
    b = _report(engine, seqs)
    assert a.tobytes() == b.tobytes()
    worst = _compare_report(a, _host_report(("squashed", F), seqs), "F = %d" % F)
    got = engine.calculate_errors(*map(np.array, seqs))
    assert list(got.keys()) == list(_host_report(("squashed", F), seqs).keys())
    with capsys.disabled():
        print("\nerror report on squashed frames, F = %d: largest relative difference to errors.calculate_errors %.3g" % (F, worst))


def test_batched_error_report_with_a_collinear_sequence(engine, capsys):
    """gem_calculate_errors_chunks on three 24-frame sequences, the middle one on ONE line in all its frames (rank 1 per frame AND
    over the sequence): rows 0 and 2 bitwise their single-sequence calls, row 1 against the host mirror and bitwise its own call."""
    import torch
    F = 24
    sets = [T.sequences(F, 31)[0], T.line_sequences(F, 32), T.sequences(F, 33)[0]]
    dev = [torch.from_numpy(np.concatenate([s[k] for s in sets])).to(engine.device) for k in range(4)]
    rows = engine.calculate_errors_chunks(*dev, 3).cpu().numpy()
    again = engine.calculate_errors_chunks(*dev, 3).cpu().numpy()
    assert rows.shape == (3, 32) and rows.tobytes() == again.tobytes()
    for i in range(3):
        single = _report(engine, sets[i])
        assert rows[i].tobytes() == single.tobytes(), (i, np.abs(rows[i] - single).max())
    S, _ = T.covariance_singular_values(sets[1][0].reshape(-1, 3), sets[1][3].reshape(-1, 3))
    assert S[1] / S[0] < 1e-15
    worst = _compare_report(rows[1], _host_report("line", sets[1]), "collinear sequence")
    with capsys.disabled():
        print("\nbatched error report, collinear sequence: largest relative difference to errors.calculate_errors %.3g" % worst)
