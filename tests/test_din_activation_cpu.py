"""CPU checks for the fused DIN local activation (csrc/din_activation.hip): the header exports,
the argument errors (no device access), the Python switches, and — on exactly the inputs the GPU
file runs — that an fp32 torch restatement stays within a quarter of the GPU bound and that the
folded form the kernels build equals the literal one in float64."""
import numpy as np
import pytest
import torch

from recommender_amd import _lib as L
from tests import din_activation_ref as R

SYMS = ("rs_din_activation_workspace_size", "rs_din_activation_fwd", "rs_din_activation_bwd")


def test_header_declares_and_library_exports_the_entry_points(lib):
    for s in SYMS:
        assert s in L.header_symbols(), s
        assert hasattr(lib, s), s


def test_workspace_size_covers_the_biases_and_partials(lib):
    n = lib.rs_din_activation_workspace_size(4096, 100, 36)
    assert n >= (3 * 36 * 80 + 4096 * 80) * 4
    assert lib.rs_din_activation_workspace_size(0, 100, 36) > 0


def _fwd(lib, p, B, Lh, D, ws_ptr, ws_bytes, null=None):
    a = [p] * 3 + [B, Lh, D] + [p] * 6 + [p, ws_ptr, ws_bytes, None]
    if null is not None:
        a[null] = None
    return lib.rs_din_activation_fwd(*a)


def _bwd(lib, p, B, Lh, D, ws_ptr, ws_bytes, null=None):
    a = [p] * 3 + [B, Lh, D] + [p] * 6 + [p] * 4 + [ws_ptr, ws_bytes, None]
    if null is not None:
        a[null] = None
    return lib.rs_din_activation_bwd(*a)


def test_argument_errors_without_gpu(lib):
    """Every refusal happens before any device access: the pointers are never dereferenced."""
    p = 4096  # a non-null address
    big = lib.rs_din_activation_workspace_size(8, 5, 36)
    for call in (_fwd, _bwd):
        assert call(lib, p, 8, 5, 7, p, big) == L.RS_E_UNSUPPORTED
        assert b"not built" in lib.rs_last_error()
        assert call(lib, p, 8, 5, 64, p, big) == L.RS_E_UNSUPPORTED
        assert call(lib, p, 8, 0, 36, p, big) == L.RS_E_INVALID      # L < 1
        assert call(lib, p, -1, 5, 36, p, big) == L.RS_E_INVALID
        assert call(lib, p, 8, 5, 36, p, big - 1) == L.RS_E_WORKSPACE
        assert b"workspace" in lib.rs_last_error()
        assert call(lib, p, 8, 5, 36, None, big) == L.RS_E_INVALID   # null workspace
    for i in (0, 1, 2, 6, 7, 8, 9, 10, 11, 12):                     # inputs, parameters, rep
        assert _fwd(lib, p, 8, 5, 36, p, big, null=i) == L.RS_E_INVALID, i
        assert b"null" in lib.rs_last_error()
    for i in (0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):         # ... drep and the gradients
        assert _bwd(lib, p, 8, 5, 36, p, big, null=i) == L.RS_E_INVALID, i


def test_python_switches_exist_and_default_off():
    from recommender_amd.dien import DIN
    from recommender_amd.dien.layers import LocalActivationUnit

    u = LocalActivationUnit(36, device="cpu")
    assert u.fused is False
    assert LocalActivationUnit(16, device="cpu", fused=True).fused is True
    with pytest.raises(ValueError, match="built for"):
        LocalActivationUnit(20, device="cpu", fused=True)
    kw = dict(item_vocab_size=50, item_embedding_size=18, cat_vocab_size=9, cat_embedding_size=18,
              mlp_units=[8, 1], device="cpu")
    assert DIN(**kw).local_activation_unit.fused is False
    assert DIN(fused_activation=True, **kw).local_activation_unit.fused is True
    with pytest.raises(ValueError):
        DIN(fused_activation=True, **{**kw, "cat_embedding_size": 10})


def test_fused_unit_on_cpu_inputs_takes_the_torch_path():
    """fused=True with inputs that are not on the GPU: the torch path, same bits as fused=False."""
    from recommender_amd.dien.layers import LocalActivationUnit

    inp = R.make_inputs(36, 5, 16, "all")
    a = LocalActivationUnit(36, device="cpu", generator=torch.Generator().manual_seed(1))
    b = LocalActivationUnit(36, device="cpu", generator=torch.Generator().manual_seed(1), fused=True)
    ra = a((inp["target"], inp["his"]), mask=inp["mask"])
    rb = b((inp["target"], inp["his"]), mask=inp["mask"])
    assert torch.equal(ra, rb)


def test_train_cli_has_the_fused_din_flag():
    import inspect

    from recommender_amd.dien import train

    assert "--fused_din" in inspect.getsource(train.main)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fp32_restatement_within_a_quarter_of_the_bound(case):
    """The fp32 torch evaluation (literal and folded) of the GPU file's inputs against float64:
    below RTOL / 4, so the GPU bound leaves room for another summation order, not for an error."""
    inp = R.make_inputs(*case)
    ref = R.reference(*case)
    for form in ("literal", "folded"):
        got = R.evaluate(inp, torch.float32, form)
        for n, g, r in zip(R.NAMES, got, ref):
            e = R.rel_err(g.numpy(), r)
            assert e <= R.RTOL / 4, f"{form} {n}: {e:.3g}"


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_folded_form_equals_the_literal_one_in_float64(case):
    inp = R.make_inputs(*case)
    ref = R.reference(*case)
    got = R.evaluate(inp, torch.float64, "folded")
    for n, g, r in zip(R.NAMES, got, ref):
        e = R.rel_err(g.numpy(), r)
        assert e <= 1e-12, f"{n}: {e:.3g}"


def test_two_round_batch_formula():
    for cus in (256, 304, 64):
        B = R.two_round_batch(cus)
        fwd, bwd = R.grid_blocks(B, cus)
        assert fwd == 3 * cus and bwd == cus and (B + 3) // 4 == 2 * fwd + 1 and B % 4 == 2


def test_saturated_inputs_reach_60_and_fp32_stays_within_a_quarter():
    inp = R.make_saturated()
    W1, b1, W2, b2 = [p.double() for p in inp["params"][:4]]
    t = inp["target"].double().expand(-1, inp["L"], -1)
    h = inp["his"].double()
    z1 = torch.cat([t, h, t - h, t * h], -1) @ W1 + b1
    z2 = torch.sigmoid(z1) @ W2 + b2
    assert abs(float(z1.abs().max()) - 60) < 1e-3 and abs(float(z2.abs().max()) - 60) < 1e-3
    ref = R.saturated_reference()
    for form in ("literal", "folded"):
        for n, g, r in zip(R.NAMES, R.evaluate(inp, torch.float32, form), ref):
            assert R.rel_err(g.numpy(), r) <= R.RTOL / 4, (form, n)
