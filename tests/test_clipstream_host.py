"""Host-only: the streamed clipped round (flearn_amd/clipstream.py, StreamedNormClip, ABI 22).  Its
refusals before a device is touched, the strategy's surface, fa_clip_fold_f32's argument and
alignment errors returned before any HIP call, the chained numpy reference (tests/clipfold_ref.py)
against clip_ref's one-pass sum for every split, and NormClip's own refusals, which stay."""
import itertools
import math
import re

import numpy as np
import pytest
import torch

import clip_ref as cr
import clipfold_ref as cf
import flearn_amd
import robust_ref as rr
import test_clip_host as tch
from flearn_amd import _native as na
from flearn_amd import clipstream
from test_clip_host import FAKE, bare_engine, header_define, nothing_launched, uploads


@pytest.fixture(scope="module")
def L():
    return na.load()


# ---------------------------------------------------------------------------------------------
# the numpy chain against the existing oracle
# ---------------------------------------------------------------------------------------------
def test_fold_chain_is_clipped_sum_for_every_split():
    rng = np.random.default_rng(3)
    n, cols = 7, 37
    g = rng.standard_normal(cols).astype(np.float32)
    x = (g + rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-2, 3, (n, 1))).astype(np.float32)
    x[:, 2], g[2] = -0.0, -0.0
    x[3, 5] = 3.0e38
    for scale in (np.array([1.0, 0.37, 0.0, 2.0, np.nan, 1e-3, -1.0], np.float32), np.ones(n, np.float32),
                  np.zeros(n, np.float32)):
        want = cr.clipped_sum(x, g, scale)
        for k in range(n):
            for splits in itertools.combinations(range(1, n), k):
                assert rr.same_bits(cf.fold_chain(x, g, scale, splits), want), splits
    assert np.signbit(cf.fold_chain(x, g, np.ones(n, np.float32), (1, 4))[2])  # -0.0 survives an opening chunk
    assert cf.chunks_of(5, (2,)) == [(0, 2), (2, 5)] and cf.chunks_of(3, ()) == [(0, 3)]
    assert cf.TARGETS == {f"clip_fold_kernel<{v},{16 // v},4,true>" for v in (1, 2, 4, 8, 16)}


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_abi_22(L):
    text = re.sub(r"/\*.*?\*/", "", tch.HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+fa_clip_fold_f32\s*\(", text)
    assert L.fa_abi_version() == header_define("FA_ABI_VERSION") == na.ABI_VERSION >= 22
    assert "fa_clip_fold_f32" in na.EXPORTS and hasattr(L, "fa_clip_fold_f32")
    tch.test_abi_surface(L)


def test_clip_fold_refusals_need_no_gpu(L):
    arg, align = header_define("FA_ERR_ARG"), header_define("FA_ERR_ALIGN")
    OTHER = FAKE + (1 << 16)

    def call(stack=FAKE, stride=64, n=5, center=FAKE, scale=FAKE, acc_in=None, acc=FAKE, col=0, ncols=64):
        rc = L.fa_clip_fold_f32(stack, stride, n, center, scale, acc_in, acc, col, ncols, None)
        nothing_launched(L)
        return rc

    for acc_in in (None, FAKE, OTHER):  # opening, in place, out of place: the same checks
        assert call(stack=None, acc_in=acc_in) == arg and call(center=None, acc_in=acc_in) == arg
        assert call(scale=None, acc_in=acc_in) == arg and call(acc=None, acc_in=acc_in) == arg
        assert b"null" in L.fa_last_error()
        assert call(n=0, acc_in=acc_in) == arg and b"n_clients" in L.fa_last_error()
        assert call(n=129, acc_in=acc_in) == arg and b"128" in L.fa_last_error()
        assert call(n=-1, acc_in=acc_in) == arg and call(n=2**31 - 1, acc_in=acc_in) == arg
        assert call(ncols=-1, acc_in=acc_in) == arg and b"window" in L.fa_last_error()
        assert call(col=-4, acc_in=acc_in) == arg and call(col=8, ncols=60, acc_in=acc_in) == arg
        big = 2**63 - 1
        assert call(col=big - 3, ncols=8, acc_in=acc_in) == arg and call(ncols=big, acc_in=acc_in) == arg
        assert call(stack=FAKE + 4, acc_in=acc_in) == align and call(stride=66, acc_in=acc_in) == align
        assert call(col=2, ncols=8, acc_in=acc_in) == align
        assert call(center=FAKE + 8, acc_in=acc_in) == align and call(scale=FAKE + 2, acc_in=acc_in) == align
        assert b"aligned" in L.fa_last_error()
        assert call(scale=FAKE + 4, ncols=0, acc_in=acc_in) == 0 and call(ncols=0, acc_in=acc_in) == 0  # a no-op
        assert call(n=0, stack=FAKE + 4, acc_in=acc_in) == arg  # an argument error wins over an alignment error
    assert call(acc=FAKE + 4) == align and call(acc_in=FAKE + 4) == align and call(acc_in=FAKE + 8, acc=OTHER) == align
    # acc_out is acc_in or does not overlap it within n_cols elements (fa_fold's rule)
    assert call(acc_in=FAKE + 16) == arg and b"overlapping" in L.fa_last_error()
    assert call(acc_in=FAKE, acc=FAKE + 16 * 15) == arg and call(acc_in=FAKE + 256 - 16) == arg
    assert call(acc_in=FAKE + 16, ncols=0) == 0  # nothing is read or written


# ---------------------------------------------------------------------------------------------
# the engine's refusals: before a device is touched
# ---------------------------------------------------------------------------------------------
def test_binding():
    from flearn_amd.aggregator import Aggregator
    from flearn_amd.streaming import RoundAccumulator

    assert Aggregator.begin_clipped_round is clipstream.begin_clipped_round
    assert Aggregator.ensemble_clipped_chunked is clipstream.ensemble_clipped_chunked
    assert issubclass(clipstream.ClippedRoundAccumulator, RoundAccumulator)
    assert hasattr(flearn_amd.ops, "clip_fold_stack")


def test_engine_refusals_touch_no_device():
    from flearn_amd.serverstate import DynState

    ups = uploads(7)
    good = {k: np.zeros_like(v) for k, v in ups[0].items()}

    def begin(agg=None, tau=1.0, center=good, **kw):
        return (agg or bare_engine()).begin_clipped_round(tau, center, **kw)

    for k in (0, -1, 129, 1000, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="chunk_clients"):
            begin(chunk_clients=k)
    with pytest.raises(ValueError, match="norm launch"):
        begin(chunk_clients=129)
    with pytest.raises(ValueError, match="group"):
        begin(bare_engine(_dist=True))
    with pytest.raises(ValueError, match="one device"):
        begin(bare_engine(devices=[torch.device("cpu")] * 2))
    with pytest.raises(ValueError, match="quantile of norms it has not seen"):
        begin(tau=None, quantile=0.5)
    with pytest.raises(ValueError, match="quantile of norms it has not seen"):
        bare_engine().ensemble_clipped_chunked(ups, None, center=good, quantile=0.5)
    for tau in (None, 0.0, -1.0, math.nan, True, "1"):
        with pytest.raises(ValueError, match="tau"):
            begin(tau=tau)
    with pytest.raises(TypeError, match="Dyn"):
        begin(server_opt=object.__new__(DynState))
    with pytest.raises(ValueError, match="center"):
        begin(center=[1, 2])
    # clip.check_noise's refusals
    for kw, word in (({"noise_multiplier": -1.0, "seed": 1}, "noise_multiplier"), ({"noise_multiplier": 1.0}, "seed"),
                     ({"noise_multiplier": 1.0, "seed": 1, "sequence": -1}, "sequence"),
                     ({"noise_multiplier": 1.0, "seed": 1, "tau": math.inf}, "finite tau"),
                     ({"noise_multiplier": 1.0, "seed": 1, "center": None}, "centre"),
                     ({"noise_multiplier": 1e30, "seed": 1, "tau": 1e30}, "sigma")):
        with pytest.raises(ValueError, match=word):
            begin(**kw)
    assert begin(noise_multiplier=0.0)._noise is None and begin(noise_multiplier=None, seed=None)._audit == {}
    # at the first upload
    with pytest.raises(TypeError, match="float16"):
        begin().add({"agg_weight": 1.0, "params": uploads(1, np.float16)[0]})
    with pytest.raises(ValueError, match="fp32 bucket"):
        begin().add({"agg_weight": 1.0, "params": uploads(1, np.float64)[0]})
    with pytest.raises(ValueError, match="fp32 bucket"):
        begin(center=None).add({"agg_weight": 1.0, "params": {"n": np.array(3, np.int64)}})
    with pytest.raises(ValueError, match="center has no key"):
        begin(center={"a.weight": good["a.weight"]}).add({"agg_weight": 1.0, "params": ups[0]})
    with pytest.raises(ValueError, match="elements"):
        begin(center=dict(good, **{"a.bias": np.zeros(4, np.float32)})).add({"agg_weight": 1.0, "params": ups[0]})
    with pytest.raises(KeyError, match="agg_weight"):  # required (and ignored)
        begin().add({"params": ups[0]})
    # later uploads: RoundAccumulator's checks
    acc = begin(chunk_clients=8)
    acc.add({"agg_weight": 0.25, "params": ups[0]})
    acc.add({"agg_weight": np.float32(3.0), "params": ups[1]})  # ignored: the round's weights are Python-int 1
    assert acc._weights == [1, 1]
    with pytest.raises(KeyError):
        acc.add({"agg_weight": 1.0, "params": {"a.weight": ups[2]["a.weight"]}})
    with pytest.raises(ValueError, match="does not match"):
        acc.add({"agg_weight": 1.0, "params": dict(ups[2], **{"a.bias": np.zeros(4, np.float32)})})
    # an empty round raises what ensemble_clipped([]) raises
    with pytest.raises(Exception) as one:
        bare_engine().ensemble_clipped([], 1.0, None, center=good)
    for run in (lambda: begin().finish(), lambda: bare_engine().ensemble_clipped_chunked([], 1.0, center=good)):
        with pytest.raises(type(one.value), match=re.escape(str(one.value))):
            run()
    # a good round gets as far as the pack, in the chunk the engine was told
    for n, k in ((7, 3), (7, 16), (2, None)):
        agg = bare_engine()
        with pytest.raises(AssertionError, match="touched its packer"):
            agg.ensemble_clipped_chunked(uploads(n), 1.0, center=good, chunk_clients=k)


def test_strategy_surface_and_refusals():
    from flearn_amd.strategy import AVG, NormClip, StreamedNormClip

    assert flearn_amd.StreamedNormClip is StreamedNormClip
    assert "StreamedNormClip" in flearn_amd.__all__ and "StreamedNormClip" in flearn_amd.strategy.__all__
    assert issubclass(StreamedNormClip, AVG) and not issubclass(StreamedNormClip, NormClip)
    assert StreamedNormClip.client is AVG.client and StreamedNormClip.client_receive is AVG.client_receive
    s = StreamedNormClip(2)
    assert (s.tau, s.center, s.server_opt, s.output, s._prev_glob, s.chunk_clients) == (2.0, "previous", None, "reference", None, 16)
    assert (s.noise_multiplier, s.sequence, s._noised) == (None, 0, False) and 0 <= s.seed < 2**64
    s = flearn_amd.setup_strategy("normclip_stream", None, tau=3.0, output="device", chunk_clients=64,
                                  noise_multiplier=1.1, seed=5, sequence=2)
    assert type(s) is StreamedNormClip
    assert (s.tau, s.output, s.chunk_clients, s.noise_multiplier, s.seed, s.sequence, s._noised) == (3.0, "device", 64, 1.1, 5, 2, True)
    assert flearn_amd.setup_strategy("NormClip_Stream", None, tau=1.0).chunk_clients == 16
    for kw in ({"tau": None}, {"tau": 0.0}, {"tau": -1.0}, {"tau": math.nan}, {"tau": True}, {"tau": 1.0, "chunk_clients": 0},
               {"tau": 1.0, "chunk_clients": 129}, {"tau": 1.0, "chunk_clients": None}, {"tau": 1.0, "chunk_clients": 2.5},
               {"tau": 1.0, "center": None}, {"tau": 1.0, "center": "mean"}, {"tau": 1.0, "noise_multiplier": -1.0},
               {"tau": math.inf, "noise_multiplier": 1.0}, {"tau": 1.0, "noise_multiplier": 1.0, "sequence": -1}):
        with pytest.raises(ValueError):
            StreamedNormClip(**kw)
    with pytest.raises(TypeError):
        StreamedNormClip(1.0, quantile=0.5)  # a fixed tau only
    with pytest.raises(ValueError, match="dict"):
        StreamedNormClip(1.0).init_global([1, 2])
    g = {"a": np.ones(3, np.float32), "b": torch.ones(2)}
    s = StreamedNormClip(1.0)
    s.init_global(g)
    g["a"][0] = 5.0
    assert s._prev_glob["a"][0] == 1.0 and s._prev_glob["b"] is not g["b"]  # a copy of its own
    doc = StreamedNormClip.__doc__.lower()
    assert "agg_weight" in doc and "fixed tau" in doc and "unit" in doc and "one device" in doc


def test_strategy_errors_take_server_exceptions_route():
    from flearn_amd.strategy import StreamedNormClip

    def rounds(n, **kw):
        return [{"agg_weight": 1.0, "params": w} for w in uploads(n, **kw)]

    good = {k: np.zeros_like(v) for k, v in uploads(7)[0].items()}
    for ups in (rounds(7, dtype=np.float16), rounds(7, dtype=np.float64),  # no fp32 bucket
                rounds(7, extra={"c": np.zeros(2, np.float32)}), []):  # a centre lacking a key; an empty round
        for streamed in (False, True):
            strat = StreamedNormClip(1.0, noise_multiplier=1.0, seed=3)
            strat.init_global(good)
            strat._engine = bare_engine(chunk_clients=strat.chunk_clients)
            with pytest.raises(SystemExit):
                if streamed:
                    handle = strat.begin_round(0)
                    for u in ups:
                        handle.add(u)
                    handle.finish()
                else:
                    strat.server(ups, 0)
            assert set(strat._prev_glob) == set(good) and strat.sequence == 0  # the centre and the sequence are kept
    strat = StreamedNormClip(1.0, noise_multiplier=1.0, seed=3)  # noise on a first round without init_global
    strat._engine = bare_engine(chunk_clients=16)
    with pytest.raises(SystemExit):
        strat.server(rounds(3), 0)
    with pytest.raises(SystemExit):
        strat.begin_round(0).add(rounds(1)[0])
    with pytest.raises(KeyError):  # agg_weight is required (and ignored)
        s = StreamedNormClip(1.0)
        s._engine = bare_engine(chunk_clients=16)
        s.server([{"params": w} for w in uploads(7)], 0)


def test_normclips_refusals_still_hold():
    tch.test_engine_refusals_touch_no_device()
    tch.test_strategy_surface_and_refusals()
    tch.test_strategy_errors_take_server_exceptions_route()
