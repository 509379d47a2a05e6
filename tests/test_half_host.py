"""float16 uploads, host side (no GPU): the numpy restatement (tests/half_ref.py) against the
fixtures captured from the reference, semantics.resolve_half against numpy's own promotion and
casts, the bucket plan of a half model, the native pack, and the C ABI of the new entry points."""
import numpy as np
import pytest
import torch

import half_ref
from flearn_amd import _native as na
from flearn_amd import bucket
from flearn_amd.semantics import KIND_F16, KIND_F64, KIND_I64, resolve, resolve_half
from golden_io import Golden, cases
from test_cabi import FAKE, declared_functions, header_define
from test_host import WEIGHT_SETS

HALF_CASES = cases("half_")


def test_fixture_inventory():
    names = set(HALF_CASES)
    for row in ("pyfloat", "np16", "np32", "np64", "torch"):
        for n in (1, 3, 10):
            assert f"half_{row}_n{n}" in names
    for must in ("half_pyint_n3", "half_pybool_n3", "half_torch_pyint_n3", "half_model_n4", "half_model_torch_n4",
                 "half_model_pyint_n4", "half_bn_n4", "half_lg_n4", "half_overflow_n7", "half_overflow_torch_n7",
                 "half_w70000_n3", "half_subnormal_n5", "half_subnormal_torch_n5"):
        assert must in names, must


@pytest.mark.parametrize("name", HALF_CASES)
def test_restatement_matches_the_reference(name):
    """half_ref.server_ensemble == the reference's output, dtype and bits (NaNs by position)."""
    g = Golden(name)
    want = g.output()
    torch_inputs = g.meta.get("input_kind") == "torch"
    got = half_ref.server_ensemble(g.weights(), g.clients(), key_lst=list(want), torch_inputs=torch_inputs)
    assert set(got) == set(want)
    for k, w in want.items():
        assert half_ref.same_bits(got[k], w), (name, k, np.asarray(got[k]).dtype, np.asarray(w).dtype)


def test_fixtures_hold_the_edge_cases():
    assert np.isinf(Golden("half_overflow_n7").output()["x"]).all()
    assert np.isinf(Golden("half_overflow_torch_n7").output()["x"]).all()
    q = Golden("half_w70000_n3").output()["x"]  # np.float16(70000) is inf: inf * x, NaN where x is +-0
    assert not np.isfinite(q).any() and np.isnan(q).any()
    q = Golden("half_subnormal_n5").output()["x"]
    assert ((np.abs(q) < 2.0**-14) & (q != 0)).sum() > 200
    # the two upload types do not compute the same thing
    a, b = Golden("half_pyfloat_n10").output()["p513"], Golden("half_torch_n10").output()["p513"]
    assert (np.asarray(a) != np.asarray(b)).sum() > 20


@pytest.mark.parametrize("name", ["half_model_n4", "half_model_torch_n4"])
def test_loaded_half_is_what_load_state_dict_stores(name):
    g = Golden(name)
    out, loaded = g.output(), g.output("loaded")
    assert loaded
    for k, w in loaded.items():
        assert half_ref.same_bits(half_ref.loaded_half(out[k]), w), (name, k)
    # through float, not a direct float64 -> float16 cast: 1 + 2^-11 + 2^-30 loads as 1.0
    q = np.array([1 + 2.0**-11 + 2.0**-30])
    p = torch.zeros(1, dtype=torch.float16)
    p.copy_(torch.from_numpy(q))
    assert half_ref.loaded_half(q)[0] == p.numpy()[0] == np.float16(1.0)
    assert q.astype(np.float16)[0] != np.float16(1.0)


# ---- semantics ------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", sorted(WEIGHT_SETS))
def test_resolve_half_agrees_with_numpy(wname):
    ws = WEIGHT_SETS[wname]
    if len({np.result_type(w, np.float16) for w in ws}) > 1:
        with pytest.raises(TypeError):
            resolve_half(ws, "numpy")
        return
    xs = [np.array([1, 2, 3], dtype=np.float16) for _ in ws]
    with np.errstate(all="ignore"):
        prods = [a * x for a, x in zip(ws, xs)]
        acc = prods[0]
        for p in prods[1:]:
            acc = acc + p
        out = np.divide(acc, np.sum(ws))
    nm = resolve_half(ws, "numpy")
    assert nm.kind == KIND_F16
    assert nm.acc_dtype == acc.dtype and nm.out_dtype == out.dtype
    assert nm.weights.dtype == acc.dtype
    assert nm.denom == float(np.sum(ws))
    for a, wc in zip(ws, nm.weights):  # the cast is numpy's: a * [1] in the product's dtype
        assert wc == (a * np.ones(1, np.float16))[0]
    want_mode = {(np.float16, np.float64): na.MODE_H16_NUMPY, (np.float16, np.float16): na.MODE_H16_NP16,
                 (np.float32, np.float32): na.MODE_H16_W32, (np.float64, np.float64): na.MODE_H16_W64}
    assert nm.mode == want_mode[(acc.dtype.type, out.dtype.type)]


def test_resolve_half_torch_rows_and_refusals():
    nm = resolve_half([0.3, 2, True], "torch")
    assert (nm.kind, nm.mode, nm.weights.dtype, nm.out_dtype) == (KIND_F16, na.MODE_H16_TORCH, np.float32, np.float64)
    assert nm.weights[0] == np.float32(0.3) and nm.denom == float(np.sum([0.3, 2, True]))
    for bad in ([np.float32(1.0)], [np.float64(1.0), 2.0], [np.float16(1.0)]):
        with pytest.raises(TypeError, match="torch float16"):
            resolve_half(bad, "torch")
    with pytest.raises(TypeError, match="promote differently"):
        resolve_half([1.0, np.float32(2.0)], "numpy")
    with pytest.raises(TypeError, match="promote differently"):
        resolve_half([np.float16(1.0), np.float64(2.0)], "numpy")
    with pytest.raises(TypeError):
        resolve_half([1.0, "x"], "numpy")
    with pytest.raises(IndexError):
        resolve_half([], "numpy")
    with pytest.raises(TypeError):  # resolve() keeps its three-dtype contract
        resolve([1.0], np.float16)


def test_weak_weight_outside_the_half_range_is_inf():
    nm = resolve_half([70000, 1.0], "numpy")
    assert np.isinf(nm.weights[0]) and nm.weights.dtype == np.float16 and nm.denom == 70001.0


# ---- plan and pack --------------------------------------------------------------------------------
def _half_model(n, as_torch=False):
    g = Golden("half_model_n4")
    cl = [dict(c) for c in g.clients()[:n]]
    if as_torch:
        cl = [{k: torch.from_numpy(np.array(v, copy=True)) for k, v in c.items()} for c in cl]
    return cl


def test_plan_of_a_half_model():
    cl = _half_model(4)
    plan = bucket.make_plan([1.0, 2.0, 0.5, 1.5], cl)
    assert set(plan.groups) == {KIND_F16, KIND_F64}  # int64 counter x float weights: float64
    g = plan.groups[KIND_F16]
    assert g.store_dtype == np.float16 and g.numerics.mode == na.MODE_H16_NUMPY
    assert g.stride % 8 == 0 and g.stride % bucket.STRIDE_ALIGN_F16 == 0
    end = 0
    for s in g.segments:
        assert s.offset % 8 == 0 and s.offset >= end and s.src_dtype == np.float16
        assert s.offset - end < 8  # packed on 16-B units, not 256-B ones
        end = s.offset + s.numel
    assert end <= g.stride
    assert [s.key for s in plan.groups[KIND_F64].segments] == ["bn1.num_batches_tracked"]
    plan_i = bucket.make_plan([3, 1, 4, 2], cl)
    assert set(plan_i.groups) == {KIND_F16, KIND_I64}


def test_plan_cache_is_keyed_on_the_input_kind():
    ws = [1.0, 2.0, 0.5, 1.5]
    pn = bucket.make_plan(ws, _half_model(4))
    pt = bucket.make_plan(ws, _half_model(4, as_torch=True))
    assert pn.groups[KIND_F16].numerics.mode == na.MODE_H16_NUMPY and pn.input_kind == "numpy"
    assert pt.groups[KIND_F16].numerics.mode == na.MODE_H16_TORCH and pt.input_kind == "torch"
    assert bucket.make_plan(ws, _half_model(4)) is pn
    assert bucket.make_plan(ws, _half_model(4, as_torch=True)) is pt
    with pytest.raises(TypeError, match="torch float16"):
        bucket.make_plan([np.float32(w) for w in ws], _half_model(4, as_torch=True))


def test_native_pack_round_trip_of_numpy_half_uploads():
    cl = _half_model(4)
    plan = bucket.make_plan([1.0, 2.0, 0.5, 1.5], cl)
    g = plan.groups[KIND_F16]
    sh = bucket.Shard(0, torch.device("cpu"), 0, g.stride)
    pieces = bucket.Packer._pieces(g, [sh])
    host = torch.full((4, g.stride), 7.0, dtype=torch.float16)
    assert bucket._NativeRows.usable(pieces, [host])
    nat = bucket._NativeRows(pieces, [host], cl, [None] * 4)
    assert nat(0, 4)
    got = host.numpy()
    for n, c in enumerate(cl):
        for s in g.segments:
            assert got[n, s.offset : s.offset + s.numel].tobytes() == np.asarray(c[s.key]).tobytes(), (n, s.key)
    # a value of another dtype under a float16 key is off the plan: nothing native, the caller falls back
    bad = [dict(c) for c in cl]
    bad[2]["fc1.bias"] = bad[2]["fc1.bias"].astype(np.float32)
    assert not bucket._NativeRows(pieces, [host], bad, [None] * 4)(0, 4)


# ---- C ABI ----------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    L = na.load()
    assert declared_functions() == sorted(na.EXPORTS)
    for name in ("fa_reduce_f16", "fa_gather_rows_f16"):
        assert name in na.EXPORTS and hasattr(L, name)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 15
    for k in ("NUMPY", "TORCH", "NP16", "W32", "W64"):
        assert header_define(f"FA_MODE_H16_{k}") == getattr(na, f"MODE_H16_{k}")


def test_reduce_f16_validates_before_touching_a_device():
    L = na.load()
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")
    ok = (FAKE, 64, 2, 0, FAKE, 2.0, 0, 8, FAKE, None, None, None)

    def call(**kw):
        names = ("stack", "stride", "n", "mode", "w", "denom", "col", "ncols", "o16", "o32", "o64", "s")
        a = dict(zip(names, ok))
        a.update(kw)
        return L.fa_reduce_f16(*[a[k] for k in names])

    assert call(col=4) == align and b"float16" in L.fa_last_error()  # col_begin not a multiple of 8
    assert call(stride=68) == align
    assert call(stack=FAKE + 2) == align
    assert call(o16=FAKE + 2) == align
    assert call(o16=None, o64=FAKE + 8) == align
    assert call(n=0) == arg
    assert call(mode=99) == arg and call(mode=-1) == arg
    assert call(o16=None) == arg and b"output" in L.fa_last_error()
    assert call(col=8, ncols=60) == arg  # window > stride
    assert call(stack=None) == arg
    assert call(ncols=0) == 0
    assert L.fa_gather_rows_f16(FAKE, 64, 0, FAKE, FAKE, 1, None) == 0
    assert L.fa_gather_rows_f16(None, 64, 2, FAKE, FAKE, 1, None) == arg
