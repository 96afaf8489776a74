"""`staged_call(...).upload` on the device: the one host-to-device copy behind `ground_call`, `lock_call`, `scale_call`, `drift_call` and
`bridge_call` hands back one view per host array, laid one behind the other as the library's tables expect them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_upload_is_one_buffer_with_a_view_per_array():
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    from globalegomocap_amd import _capi
    from globalegomocap_amd._binding import staged_call
    host = [np.array([3, -1, 2 ** 40], dtype=np.int64), np.arange(6, dtype=np.float64).reshape(2, 3) / 7.0, np.array([1, 2, 3, 254, 255], dtype=np.uint8)]
    side = torch.cuda.Stream()
    with staged_call(_capi.load_library(), "cuda:0", side) as call:
        assert torch.cuda.current_stream() == side and call.stream == side
        views = call.upload(*host)
        work = call.work(24)
    side.synchronize()
    assert len(views) == 3 and work.dtype == torch.float64 and work.numel() * 8 >= 24
    for a, v in zip(host, views):
        assert v.is_cuda and tuple(v.shape) == a.shape and v.dtype == torch.from_numpy(a).dtype
        assert np.array_equal(v.cpu().numpy(), a)
    at = [v.data_ptr() for v in views]
    assert at[1] - at[0] == host[0].nbytes == 24 and at[2] - at[1] == host[1].nbytes == 48
    assert at[0] % 8 == 0 and at[1] % 8 == 0
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1          # (views of ONE uploaded buffer)
    with staged_call(_capi.load_library(), torch.device("cuda", 0)) as call:          # no stream given: the device's current one
        assert call.stream == torch.cuda.current_stream(0)
