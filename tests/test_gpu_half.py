"""GPU parity of float16 uploads (fa_reduce_f16 and the engine above it).

Oracle: tests/half_ref.py, the numpy restatement that tests/test_half_host.py pins to the fixtures
captured from the reference (tests/golden/half_*.npz).  Rule: finite values and infinities bit for
bit, NaNs by position — for out64, out32 and out16 alike.  Shapes: the 16-B unit (8 halves), the
1-KiB wave chunk (512), one piece +- 1 column, every piece width the geometry chooses, more pieces
than blocks; client counts around the pipeline depth D of the kernel each width runs.  Where a test
claims the shape it reaches, fa_last_launch must name it: the expected instantiation comes from
plan_f16_window's rule (instantiation_cases.plan_f16, held to the header by
tests/test_geometry_plan.py) on the device's CU count.  tests/test_gpu_half_instantiations.py
reaches every instantiation at small widths on a forced grid."""
import numpy as np
import pytest
import torch

import half_ref
from flearn_amd import AVG, AVGM, BN, LG, Dyn
from flearn_amd import _native as na
from flearn_amd import aggregator as agg
from flearn_amd import semantics
from golden_io import Golden, cases
from instantiation_cases import h16_name, h16_plan_name

pytestmark = pytest.mark.gpu

MODES = {
    "numpy": na.MODE_H16_NUMPY,
    "torch": na.MODE_H16_TORCH,
    "np16": na.MODE_H16_NP16,
    "w32": na.MODE_H16_W32,
    "w64": na.MODE_H16_W64,
}
VMAX = {"numpy": 16, "torch": 16, "np16": 16, "w32": 8, "w64": 4}
SENTINEL = 96  # elements after every output that must stay untouched


def weights_for(mode_name, n):
    """Non-representable weights of the mode's Python type, resolved as the engine resolves them."""
    vals = [0.3 + 1.4 * ((7 * i) % 11) / 11 for i in range(n)]
    typ = {"numpy": float, "torch": float, "np16": np.float16, "w32": np.float32, "w64": np.float64}[mode_name]
    num = semantics.resolve_half([typ(v) for v in vals], "torch" if mode_name == "torch" else "numpy")
    assert num.mode == MODES[mode_name]
    return num


def device_weights(num, cuda):
    w = num.weights.astype(np.float64 if num.mode == na.MODE_H16_W64 else np.float32)
    return torch.from_numpy(w).to(cuda)


def make_stack(n, stride, seed):
    """Normal values around 1 with the edge cases sprinkled in: subnormals, +-0, values near the top
    of the half range (sums overflow to inf), inf and NaN."""
    if stride > 70_000:  # wide stacks repeat a 65,544-column block (the arithmetic is per column)
        return np.ascontiguousarray(np.tile(make_stack(n, 65_544, seed), (1, stride // 65_544 + 1))[:, :stride])
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, stride)).astype(np.float16)
    k = rng.integers(0, 16, size=(n, stride))
    x = np.where(k == 0, (rng.standard_normal((n, stride)) * 3e-6).astype(np.float16), x)  # subnormals
    x = np.where(k == 1, np.float16(-0.0), x)
    cols = rng.integers(0, 97, size=stride)
    x[:, cols == 0] = np.float16(60000.0)  # overflows after a few clients
    x[0, cols == 1] = np.float16(np.inf)
    x[n - 1, cols == 2] = np.float16(np.nan)
    return np.ascontiguousarray(x.astype(np.float16))


def run_kernel(cuda, mode, x, num, col_begin, n_cols, outs=("out64", "out32", "out16")):
    L = na.load()
    n, stride = x.shape
    xd = torch.from_numpy(x.view(np.int16)).to(cuda)
    wd = device_weights(num, cuda)
    bufs = {
        "out16": torch.full((n_cols + SENTINEL,), 0x1234, dtype=torch.int16, device=cuda),
        "out32": torch.full((n_cols + SENTINEL,), -7.0, dtype=torch.float32, device=cuda),
        "out64": torch.full((n_cols + SENTINEL,), -7.0, dtype=torch.float64, device=cuda),
    }
    ptr = {k: (bufs[k].data_ptr() if k in outs else None) for k in bufs}
    rc = L.fa_reduce_f16(xd.data_ptr(), stride, n, mode, wd.data_ptr(), num.denom, col_begin, n_cols, ptr["out16"],
                         ptr["out32"], ptr["out64"], na.stream_handle(cuda))
    na.check(rc, "fa_reduce_f16")
    torch.cuda.synchronize()
    got = {k: bufs[k].cpu().numpy() for k in outs}
    if "out16" in got:
        got["out16"] = got["out16"].view(np.float16)
    return got


def check(cuda, mode_name, x, col_begin=0, n_cols=None, outs=("out64", "out32", "out16")):
    n, stride = x.shape
    n_cols = stride - col_begin if n_cols is None else n_cols
    num = weights_for(mode_name, n)
    got = run_kernel(cuda, MODES[mode_name], x, num, col_begin, n_cols, outs)
    launch = agg.last_launch()
    q = half_ref.reduce_rows(MODES[mode_name], np.ascontiguousarray(x[:, col_begin : col_begin + n_cols]), num.weights,
                             num.denom)
    assert q.dtype == num.out_dtype
    want = dict(zip(("out64", "out32", "out16"), half_ref.outputs(q)))
    for k in outs:
        assert half_ref.same_bits(got[k][:n_cols], want[k]), (mode_name, k, x.shape, col_begin, n_cols)
        tail = got[k][n_cols:]
        fill = np.int16(0x1234).view(np.float16) if k == "out16" else -7.0
        assert (tail == fill).all(), (mode_name, k, "stored past the window")
    return launch


def round_up(v, m):
    return (v + m - 1) // m * m


@pytest.fixture(scope="module")
def cus(cuda):
    return torch.cuda.get_device_properties(cuda).multi_processor_count


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("p", [1, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025])
def test_widths(cuda, mode_name, p):
    """The 16-B unit, the 1-KiB chunk = one single-wave piece, +- 1 column, two pieces."""
    launch = check(cuda, mode_name, make_stack(3, round_up(p, 8), seed=p))
    chunks = -(-p // 512)  # at most 3: one single-wave block per chunk on any device
    assert launch == (h16_name(MODES[mode_name], 1, 16, 1), chunks, 1)


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("n", [1, 2, 16, 17, 31, 32, 33, 100])
def test_depths_single_wave_pieces(cuda, mode_name, n):
    """N around D = 16, the depth of the one-chunk-per-block kernel a 513-column window runs."""
    launch = check(cuda, mode_name, make_stack(n, 520, seed=n))
    assert launch == (h16_name(MODES[mode_name], 1, 16, 1), 2, 1)


@pytest.mark.parametrize("mode_name", list(MODES))
def test_more_pieces_than_three_quarters_of_the_cus(cuda, cus, mode_name):
    """A grid's worth of one-chunk pieces + 1 column: the first window on 4-wave blocks (V = 1)."""
    grid = int(cus * 0.75 + 0.5)
    p = grid * 512 + 1
    launch = check(cuda, mode_name, make_stack(17, round_up(p, 8), seed=3))
    assert launch == (h16_name(MODES[mode_name], 1, 16, 4), grid, 1)
    assert launch[:2] == h16_plan_name(MODES[mode_name], round_up(p, 8), cus)


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("v", [1, 2, 4, 8, 16, 32])
def test_every_piece_width(cuda, cus, mode_name, v):
    """Shares of 4v chunks per block: 4-wave pieces of v KiB per wave, D = 16/v rows deep (v = 32:
    past one round of the widest piece, so blocks sweep several pieces), an odd column count,
    N = 2D + 1 and N = 1.  Modes with wider sums stop at their widest piece and sweep more pieces."""
    grid = int(cus * 0.75 + 0.5)
    p = grid * 4 * v * 512 - 1029  # a ragged, odd end inside the last block's piece
    vk = min(v, VMAX[mode_name])  # the piece the kernel runs: v KiB per wave, at most the mode's widest
    d = max(1, 16 // vk)
    want = h16_plan_name(MODES[mode_name], round_up(p, 8), cus)
    assert want[0] == h16_name(MODES[mode_name], vk, d, 4), want  # what the docstring claims, on this CU count
    assert (-(-round_up(p, 8) // 512) > want[1] * 4 * vk) == (v > vk)  # several pieces per block
    for n in (2 * d + 1, 1):
        launch = check(cuda, mode_name, make_stack(n, round_up(p, 8), seed=v),
                       outs=("out64", "out16") if v < 32 else ("out16",))
        assert launch == want + (1,)


@pytest.mark.parametrize("mode_name", list(MODES))
def test_window_inside_wider_rows(cuda, mode_name):
    """Odd n_cols, non-zero col_begin, row_stride > n_cols; the halves around the window are NaN in
    every row: the neighbour that an odd window's last dword brings along never reaches an output."""
    x = make_stack(9, 2048, seed=11)
    col_begin, n_cols = 520, 777
    x[:, :col_begin] = np.float16(np.nan)
    x[:, col_begin + n_cols :] = np.float16(np.nan)
    check(cuda, mode_name, x, col_begin, n_cols)
    for outs in (("out16",), ("out32",), ("out64",)):  # each output alone (the others NULL)
        check(cuda, mode_name, x, col_begin, n_cols, outs)


def test_overflow_weight_inf_and_subnormals(cuda):
    """Seven clients, weight 600 x value 30: inf.  A weak weight 70000 is inf as a half; times 0 the
    result is NaN.  Values x 1e-4 with weights < 1: subnormal products and sums are kept."""
    for ws, fill, mode in (([600] * 7, 30.0, "numpy"), ([70000, 1.0, 1.0], 0.0, "numpy"), ([600.0] * 7, 30.0, "torch")):
        num = semantics.resolve_half(ws, "torch" if mode == "torch" else "numpy")
        x = np.full((len(ws), 16), fill, dtype=np.float16)
        got = run_kernel(cuda, num.mode, x, num, 0, 16)
        q = half_ref.reduce_rows(num.mode, x, num.weights, num.denom)
        assert np.isinf(q).all() or np.isnan(q).all()
        for k, w in zip(("out64", "out32", "out16"), half_ref.outputs(q)):
            assert half_ref.same_bits(got[k][:16], w), (ws, k)
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((5, 4096)) * 1e-4).astype(np.float16)
    for mode, kind in (("numpy", "numpy"), ("torch", "torch")):
        num = semantics.resolve_half([0.11, 0.7, 0.05, 0.9, 0.33], kind)
        got = run_kernel(cuda, num.mode, x, num, 0, 4096)
        q = half_ref.reduce_rows(num.mode, x, num.weights, num.denom)
        o16 = half_ref.outputs(q)[2]
        sub = (np.abs(o16) < 6.1e-5) & (o16 != 0)
        assert sub.sum() > 100  # the case is subnormal-heavy
        for k, w in zip(("out64", "out32", "out16"), half_ref.outputs(q)):
            assert half_ref.same_bits(got[k][:4096], w), (mode, k)


def test_misaligned_window_is_refused_without_a_launch(cuda):
    L = na.load()
    x = torch.zeros((2, 64), dtype=torch.int16, device=cuda)
    w = torch.ones(2, dtype=torch.float32, device=cuda)
    out = torch.full((64,), 0x1234, dtype=torch.int16, device=cuda)
    s = na.stream_handle(cuda)
    assert L.fa_reduce_f16(x.data_ptr(), 64, 2, 0, w.data_ptr(), 2.0, 4, 8, out.data_ptr(), None, None, s) == na.FA_ERR_ALIGN
    assert L.fa_reduce_f16(x.data_ptr(), 60, 2, 0, w.data_ptr(), 2.0, 0, 8, out.data_ptr(), None, None, s) == na.FA_ERR_ALIGN
    assert L.fa_reduce_f16(x.data_ptr() + 2, 56, 2, 0, w.data_ptr(), 2.0, 0, 8, out.data_ptr(), None, None, s) == na.FA_ERR_ALIGN
    assert L.fa_reduce_f16(x.data_ptr(), 64, 2, 9, w.data_ptr(), 2.0, 0, 8, out.data_ptr(), None, None, s) == na.FA_ERR_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x1234).all()


def test_gather_rows_f16(cuda):
    """fa_gather_rows_f16: per-(client, key) device tensors at any element offset into the stack."""
    L = na.load()
    n, stride = 5, 128
    rng = np.random.default_rng(4)
    lens, cols = [1, 9, 37], [0, 8, 24]
    vals = [[rng.standard_normal(m).astype(np.float16) for m in lens] for _ in range(n)]
    # odd element offsets: views one element into a longer tensor
    dev = [[torch.from_numpy(np.concatenate([[np.float16(9)], v])).to(cuda)[1:] for v in row] for row in vals]
    ptrs = torch.tensor([dev[i][s].data_ptr() for s in range(3) for i in range(n)], dtype=torch.int64, device=cuda)
    segs = torch.tensor(cols + lens, dtype=torch.int64, device=cuda)
    stack = torch.zeros((n, stride), dtype=torch.float16, device=cuda)
    na.check(L.fa_gather_rows_f16(stack.data_ptr(), stride, n, ptrs.data_ptr(), segs.data_ptr(), 3,
                                  na.stream_handle(cuda)), "gather f16")
    got = stack.cpu().numpy()
    for i in range(n):
        want = np.zeros(stride, dtype=np.float16)
        for c, v in zip(cols, vals[i]):
            want[c : c + len(v)] = v
        assert got[i].tobytes() == want.tobytes(), i


# ---------------------------------------------------------------------------------------------
# the engine: fixtures captured from the reference through Aggregator and the strategies
# ---------------------------------------------------------------------------------------------
HALF_CASES = cases("half_")


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _uploads(g, where, cuda):
    """The case's uploads as captured ("host": numpy arrays, or torch CPU tensors for the torch
    cases) or as device tensors ("device": torch cases only — device tensors compute what CPU
    tensors do)."""
    clients = g.clients()
    if where == "device":
        clients = [{k: v.to(cuda) for k, v in c.items()} for c in clients]
    return clients


def _strategy(g, **kw):
    if g.name.startswith("half_bn"):
        return BN(**kw)
    if g.name.startswith("half_lg"):
        return LG(g.meta["shared_key_layers"], **kw)
    return AVG(**kw)


def _variants():
    for name in HALF_CASES:
        yield name, "host"
        if "torch" in name:
            yield name, "device"


@pytest.mark.parametrize("name,where", list(_variants()))
def test_fixtures_through_the_strategies(cuda, name, where):
    """AVG / BN / LG .server on every fixture, in the three output modes: "reference" has the
    reference's dtypes and bits; "float32" and "device" hold what load_state_dict ends up with,
    float16 fl16(fl32(q)) for the float16 keys."""
    g = Golden(name)
    want = g.output()
    ws = g.weights()

    def ups():
        return [{"agg_weight": w, "params": c} for w, c in zip(ws, _uploads(g, where, cuda))]

    s = _strategy(g)
    got = s.server(ups(), 0)["w_glob"]
    assert set(got) == set(want)
    for k, w in want.items():
        if where == "host" and "torch" in name:
            assert isinstance(got[k], torch.Tensor) and got[k].device.type == "cpu"
        assert half_ref.same_bits(_host(got[k]), np.asarray(w)), (name, where, k, _host(got[k]).dtype)
    assert (s.engine.last_plan.groups["f16"].numerics.mode == na.MODE_H16_TORCH) == ("torch" in name)
    half_keys = [k for k in want if _host(_uploads(g, "host", cuda)[0][k]).dtype == np.float16]
    assert half_keys
    for output in ("float32", "device"):
        got = _strategy(g, output=output).server(ups(), 0)["w_glob"]
        assert set(got) == set(want)
        for k in half_keys:
            v = got[k]
            if output == "device":
                assert isinstance(v, torch.Tensor) and v.device.type == "cuda" and v.dtype == torch.float16
            assert half_ref.same_bits(_host(v), half_ref.loaded_half(np.asarray(want[k]))), (name, where, output, k)


def test_device_uploads_take_one_gather(cuda):
    g = Golden("half_model_torch_n4")
    clients = _uploads(g, "device", cuda)
    s = AVG()
    s.server([{"agg_weight": w, "params": c} for w, c in zip(g.weights(), clients)], 0)
    assert s.engine.packer.last_row_tables.get("f16") == "gather", s.engine.packer.last_row_tables


def test_aggregator_ensemble_key_list_and_plan_reuse(cuda):
    g = Golden("half_model_n4")
    a = agg.Aggregator()
    keys = ["fc2.weight", "bn1.num_batches_tracked", "conv1.bias"]
    for _ in range(2):  # the second round reuses the plan, the staging and the cached weights
        got = a.ensemble(g.weights(), g.clients(), keys)
        assert list(got) == keys
        for k in keys:
            assert half_ref.same_bits(_host(got[k]), np.asarray(g.output()[k])), k


@pytest.mark.parametrize("fast", [True, False])
def test_http_mode_round_trip(cuda, fast):
    """Encrypt.encode per upload, receive_processing, server: float16 uploads arrive as numpy arrays."""
    from flearn_amd.wire import Encrypt

    g = Golden("half_model_n4")
    enc = Encrypt(fast_min_chars=0 if fast else None)
    strs = [enc.encode({"agg_weight": w, "params": c}) for w, c in zip(g.weights(), g.clients())]
    s = AVG(encrypt=enc)
    got = s.server([s.receive_processing(x) for x in strs], 0)["w_glob"]
    for k, w in g.output().items():
        assert half_ref.same_bits(_host(got[k]), np.asarray(w)), k
    back = enc.decode(enc.encode({"w_glob": got}))["w_glob"]
    for k, w in g.output().items():
        assert half_ref.same_bits(np.asarray(back[k]), np.asarray(w)), k


def test_unsupported_float16_rounds_raise_before_any_launch(cuda):
    g = Golden("half_model_n4")
    ws, clients = g.weights(), g.clients()
    ups = [{"agg_weight": w, "params": c} for w, c in zip(ws, clients)]
    a = agg.Aggregator()
    with pytest.raises(TypeError, match="float16"):
        a.ensemble(ws, clients, server_opt=agg.ServerOptimizer("avgm"))
    with pytest.raises(TypeError, match="float16"):
        a.ensemble(ws, clients, server_opt=agg.DynState({k: np.asarray(v) for k, v in clients[0].items()}))
    with pytest.raises(TypeError, match="float16"):
        agg.Aggregator(devices=[cuda, cuda]).ensemble(ws, clients)
    tl = [{k: torch.from_numpy(np.array(v, copy=True)) for k, v in c.items()} for c in clients]
    with pytest.raises(TypeError, match="torch float16"):
        a.ensemble([np.float32(w) for w in ws], tl)
    with pytest.raises(TypeError, match="promote differently"):
        a.ensemble([1.0, np.float32(2), 1.0, 1.0], clients)
    bf = [{"x": torch.ones(8, dtype=torch.bfloat16)} for _ in range(2)]
    with pytest.raises(TypeError):  # bfloat16 keeps raising (the reference exits on it too)
        a.ensemble([1.0, 1.0], bf)
    for s in (AVGM(server_side=True), Dyn({k: np.asarray(v) for k, v in clients[0].items()})):
        with pytest.raises(SystemExit):  # the reference's server_exception route
            s.server(ups, 0)
    # nothing above left a launch behind: the next plain round is exact
    got = a.ensemble(ws, clients)
    for k, w in g.output().items():
        assert half_ref.same_bits(_host(got[k]), np.asarray(w)), k
