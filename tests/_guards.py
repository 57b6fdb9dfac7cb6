"""What the per-element bound tests on the device share (test_norm_bounds_gpu.py, test_image_bounds_gpu.py): the
fixture that loads the native library and pins its switches, the dispatch-counter assertion, and the guarded
buffers that show a kernel writes only its own output."""
import pytest
import torch

from comfy_gen_server_amd import ops, _native

GN_BLOCKS = 2048                     # the default of CGS_GN_BLOCKS


@pytest.fixture(autouse=True)
def _native_loaded(cuda, monkeypatch):
    lib = _native.load_kernels()
    assert lib is not None, _native.kernels_error()
    monkeypatch.setenv("CGS_AUTOTUNE", "0")
    lib.cgs_gn_set_blocks(GN_BLOCKS)
    lib.cgs_dwconv_set_px(4)
    ops.reset_stats()
    yield


def _ran_native(op, n=1):
    st = ops.stats()
    assert st.get((op, "hip"), 0) == n and not any(key[1] == "lib" for key in st), st
    ops.reset_stats()


# ---- a kernel writes only its own output
GUARD = 4096


def _guarded(cuda, numel, slack):
    """numel 16-bit elements of output in the middle of an int16 pattern: GUARD before, slack after."""
    n = GUARD + numel + slack
    buf = ((torch.arange(n, device=cuda, dtype=torch.int64) * 2654435761 >> 7) & 0x7FFF).to(torch.int16)
    return buf, buf.clone(), buf.data_ptr() + 2 * GUARD


def _guarded32(cuda, numel, slack):
    """_guarded for 32-bit elements (fp32 outputs): an int32 pattern, the pointer 4 GUARD bytes in."""
    n = GUARD + numel + slack
    buf = ((torch.arange(n, device=cuda, dtype=torch.int64) * 2654435761 >> 7) & 0x7FFFFFFF).to(torch.int32)
    return buf, buf.clone(), buf.data_ptr() + 4 * GUARD


def _check_guard(buf, before, keep, dtype, what):
    """``keep``: a bool mask over buf[GUARD:] of the elements the kernel may write. Returns them as ``dtype``."""
    torch.cuda.synchronize()
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[GUARD:GUARD + keep.numel()] = keep.reshape(-1)
    changed = ((buf != before) & ~mask).nonzero().flatten()
    assert changed.numel() == 0, (f"{what}: {changed.numel()} elements outside the output changed, first at buffer "
                                  f"offset {int(changed[0])} (the output starts at {GUARD})")
    return buf[mask].view(dtype)
