"""The mask normalisation of ops.attention (attention_mask_layout: pure, shape / strides / dtype in and out) and the
untouched torch path of masked attention on the CPU."""
import math

import pytest
import torch

from comfy_gen_server_amd import ops
from comfy_gen_server_amd.ops import core
from comfy_gen_server_amd.ops.core import attention_mask_layout

B, H, Sq, Sk = 3, 5, 16, 64
BF = torch.bfloat16


def _contig(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= d
    return tuple(reversed(st))


@pytest.mark.parametrize("shape,shape4,strides4", [
    ((Sq, Sk), (1, 1, Sq, Sk), (0, 0, Sk, 1)),
    ((B, Sq, Sk), (B, 1, Sq, Sk), (Sq * Sk, 0, Sk, 1)),
    ((1, Sq, Sk), (1, 1, Sq, Sk), (0, 0, Sk, 1)),
    ((B, H, Sq, Sk), (B, H, Sq, Sk), (H * Sq * Sk, Sq * Sk, Sk, 1)),
    ((1, H, Sq, Sk), (1, H, Sq, Sk), (0, Sq * Sk, Sk, 1)),
    ((B, 1, Sq, Sk), (B, 1, Sq, Sk), (Sq * Sk, 0, Sk, 1)),
    ((1, 1, Sq, Sk), (1, 1, Sq, Sk), (0, 0, Sk, 1)),
    ((B, 1, 1, Sk), (B, 1, 1, Sk), (Sk, 0, 0, 1)),
])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_layout_accepted_forms_pass_as_they_are(shape, shape4, strides4, dtype):
    got = attention_mask_layout(shape, _contig(shape), dtype, B, H, Sq, Sk)
    assert got == (shape4, strides4, dtype, False)


@pytest.mark.parametrize("dtype,kdtype", [(torch.bool, BF), (torch.float16, torch.float32)])
def test_layout_converted_dtypes_copy_at_own_shape(dtype, kdtype):
    shape = (B, 1, Sq, 77)
    got = attention_mask_layout(shape, _contig(shape), dtype, B, H, Sq, 77)
    assert got == (shape, (Sq * 80, 0, 80, 1), kdtype, True)          # rows padded to 80 keys, head not expanded


def test_layout_size_one_dims_get_stride_zero_whatever_their_stride():
    got = attention_mask_layout((1, 1, Sq, Sk), (12345, 777, Sk, 1), BF, B, H, Sq, Sk)
    assert got == ((1, 1, Sq, Sk), (0, 0, Sk, 1), BF, False)
    # an expanded view already has stride 0 on its broadcast dims: stays, no copy
    got = attention_mask_layout((B, H, Sq, Sk), (0, 0, Sk, 1), torch.float32, B, H, Sq, Sk)
    assert got == ((B, H, Sq, Sk), (0, 0, Sk, 1), torch.float32, False)


@pytest.mark.parametrize("shape,strides,aligned", [
    ((Sq, 77), (77, 1), True),                      # rows not a multiple of 4 elements apart
    ((Sq, Sk), (Sk + 24, 1), False),                # a column slice whose base is not 16-byte aligned
    ((Sq, Sk), (1, Sq), True),                      # transposed: key stride not 1
    ((B, Sq, Sk), (Sq * Sk + 2, Sk, 1), True),      # batch stride not a multiple of 4
])
def test_layout_unaligned_masks_copy_padded(shape, strides, aligned):
    sk = shape[-1]
    row = (sk + 7) // 8 * 8
    shape4, strides4, kdtype, copy = attention_mask_layout(shape, strides, BF, B, H, Sq, sk, aligned)
    assert copy and kdtype == BF and strides4[2:] == (row, 1)
    assert shape4 == ((1, 1) + shape if len(shape) == 2 else (shape[0], 1) + shape[1:])
    assert strides4[0] == (0 if shape4[0] == 1 else Sq * row) and strides4[1] == 0


def test_layout_aligned_column_slice_is_not_copied():
    got = attention_mask_layout((Sq, Sk), (Sk + 24, 1), BF, B, H, Sq, Sk, True)
    assert got == ((1, 1, Sq, Sk), (0, 0, Sk + 24, 1), BF, False)


@pytest.mark.parametrize("shape", [(Sq + 1, Sk), (B + 1, Sq, Sk), (B, H + 1, Sq, Sk), (B, H, Sq, Sk + 1), (Sk,),
                                   (1, B, H, Sq, Sk), (2, Sq, Sk)])
def test_layout_rejects_shapes_that_do_not_broadcast(shape):
    with pytest.raises(ValueError):
        attention_mask_layout(shape, _contig(shape), torch.float32, B, H, Sq, Sk)


def test_layout_rejects_integer_masks():
    with pytest.raises(ValueError):
        attention_mask_layout((Sq, Sk), (Sk, 1), torch.int64, B, H, Sq, Sk)


@pytest.mark.parametrize("shape,dtype", [((Sq, 77), torch.float32), ((B, Sq, 77), BF), ((1, H, Sq, 77), BF),
                                         ((B, H, Sq, 77), torch.float32), ((B, 1, Sq, 77), torch.bool),
                                         ((B, 1, Sq, 77), torch.float16)])
def test_cpu_masked_attention_is_the_reference(shape, dtype):
    D = 8
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, Sq, H * D, generator=g)
    k, v = torch.randn(B, 77, H * D, generator=g), torch.randn(B, 77, H * D, generator=g)
    blocked = torch.rand(shape, generator=g) < 0.3
    blocked[..., 0] = False
    if dtype == torch.bool:
        mask = ~blocked
    else:
        mask = (torch.randint(-16, 17, shape, generator=g).float() / 4).masked_fill(blocked, -math.inf).to(dtype)
    ops.reset_stats()
    o = ops.attention(q, k, v, H, mask=mask)
    assert ops.stats() == {("attention", "torch"): 1}
    assert torch.equal(o, core.attention_reference(q, k, v, H, mask=mask))
