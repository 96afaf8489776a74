"""The tensor-argument check every entry point of the binding shares (`_binding.check_tensor`, `check_tensors`), on host tensors: what
is not a device tensor is refused first, so no device is needed to see the refusals; for the shape forms a host tensor that says it is
on the device stands in for one (the check reads `is_cuda`, the dtype, the shape and the strides, never the data)."""
import pytest
import torch

from globalegomocap_amd._binding import check_tensor, check_tensors


class _SaysDevice(torch.Tensor):
    is_cuda = True


def _device(*shape, dtype=torch.float64):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_SaysDevice)


def test_none_is_an_argument_not_given():
    check_tensors("entry", (None, torch.float64, (7, 15, 3)), (None, torch.int32, None))
    with pytest.raises(TypeError, match="entry wants contiguous device tensors of the documented dtypes"):
        check_tensor(None, torch.float64, what="entry")          # (the single check is for a required argument)


def test_what_is_no_device_tensor_is_a_type_error():
    for x in ([[0.0] * 3] * 15, torch.zeros(7, 15, 3, dtype=torch.float64)):          # a Python list; a host tensor of the right shape
        with pytest.raises(TypeError, match="entry wants contiguous device tensors of the documented dtypes"):
            check_tensors("entry", (x, torch.float64, (7, 15, 3)))
        with pytest.raises(TypeError, match="entry wants"):
            check_tensor(x, torch.float64, (None, 15, 3), what="entry")
    with pytest.raises(TypeError, match="entry wants"):
        check_tensor(_device(7, 15, 3, dtype=torch.float32), torch.float64, what="entry")          # the wrong dtype
    with pytest.raises(TypeError, match="entry wants"):
        check_tensor(_device(7, 3, 15).transpose(1, 2), torch.float64, (7, 15, 3), what="entry")          # not contiguous


def test_the_caller_words_the_refusals():
    with pytest.raises(ValueError, match="^my words$"):
        check_tensor([1.0], torch.float64, error=ValueError("my words"))
    with pytest.raises(ValueError, match="^my words$"):          # (one error given: it stands for the shape as well)
        check_tensor(_device(7, 15, 2), torch.float64, (None, 15, 3), error=ValueError("my words"))
    with pytest.raises(ValueError, match="^the shape$"):
        check_tensor(_device(7, 15, 2), torch.float64, (None, 15, 3), error=TypeError("the tensor"), shape_error=ValueError("the shape"))


def test_a_shape_with_free_leading_dimensions():
    for frames in (0, 7):
        check_tensor(_device(frames, 15, 3), torch.float64, (None, 15, 3), what="entry")
    with pytest.raises(ValueError, match=r"entry: a tensor of shape \(7, 15, 2\) where \(None, 15, 3\) is expected"):
        check_tensor(_device(7, 15, 2), torch.float64, (None, 15, 3), what="entry")
    with pytest.raises(ValueError, match="entry: a tensor of shape"):
        check_tensor(_device(105, 3), torch.float64, (None, 15, 3), what="entry")          # (the right size in the wrong rank)
    check_tensors("entry", (_device(7, 15, 3), torch.float64, (7, 15, 3)))
    with pytest.raises(ValueError, match=r"entry: a tensor of shape \(7, 15, 3\) where \(8, 15, 3\) is expected"):
        check_tensors("entry", (_device(7, 15, 3), torch.float64, (8, 15, 3)))


def test_the_element_counts():
    n = 48
    check_tensor(_device(n, dtype=torch.uint8), torch.uint8, at_least=n, what="entry")
    check_tensor(_device(n + 16, dtype=torch.uint8), torch.uint8, at_least=n, what="entry")
    with pytest.raises(ValueError, match="^too small$"):
        check_tensor(_device(n - 1, dtype=torch.uint8), torch.uint8, at_least=n, error=ValueError("too small"))
    check_tensor(_device(13), torch.float64, numel=13, what="entry")
    for m in (12, 14):
        with pytest.raises(TypeError, match="^13 values$"):
            check_tensor(_device(m), torch.float64, numel=13, error=TypeError("13 values"))


def test_rows_with_a_stride_of_their_own():
    wide = _device(5, 64, dtype=torch.uint8)
    check_tensor(wide[:, :48], torch.uint8, rows=(5, 40), what="entry")          # rows 64 bytes apart, 48 wide: not contiguous, and fine
    check_tensor(wide, torch.uint8, rows=(5, 64), what="entry")
    strided = _device(5, 128, dtype=torch.uint8)[:, ::2]
    for bad in (wide[:, :32], wide[:4], strided, _device(5 * 64, dtype=torch.uint8)):          # too narrow, too few, strided, flat
        with pytest.raises(ValueError, match="^rows$"):
            check_tensor(bad, torch.uint8, rows=(5, 40), error=ValueError("rows"))
