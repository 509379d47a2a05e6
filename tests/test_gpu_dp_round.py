"""GPU: DP-FedAvg rounds through the strategy (NormClip(noise_multiplier=...) ->
Aggregator.ensemble_clipped -> ops.gauss_add).

Without noise the round is the parent's, bit for bit.  With noise the expected value is derived, not
measured.  The scales follow from the device's norms (engine.last_clip["norm2"], held to their bound
by tests/test_gpu_clip_round.py) and the clipped sum S is clip_ref's, which the device matches bit for
bit.  The device then holds acc = fl32(S + fl32(sigma * z_gpu)) per column, and the reference value is
S + sigma * z_ref in float64 (sigma the fp32 value).  With u = 2^-24, E = noise_ref.Z_ERROR and
zz = |z_ref| + E >= |z_gpu|:

    |sigma * z_gpu - sigma * z_ref|            <= sigma * E                (the transform, measured once)
    |fl32(sigma * z_gpu) - sigma * z_gpu|      <= u * sigma * zz + 2^-150  (the product's rounding)
    |acc - (S + fl32(sigma * z_gpu))|          <= u * (|S| + sigma * zz * (1 + u) + 2^-150)   (the add's)

The float64 divide by N adds 2^-53 relative; the fp32 outputs round once more (u relative); a first
FedAVGM step from v = 0 computes d = g - l, v = d + 0, w = l + v in float64: two more roundings of
at most 2^-53 * (|g| + |l|) each."""
import numpy as np
import pytest

import clip_ref as cr
import noise_ref as nr
import robust_ref as rr
from flearn_amd import NormClip, clip
from flearn_amd.aggregator import ServerOptimizer
from golden_io import Golden
from test_gpu_clip_round import OUTPUTS, _host, f32_keys, make_round, norms_of, same, upload

pytestmark = pytest.mark.gpu

N = 10
SEED = 0x5EEDC0FFEE123457
U = 2.0 ** -24
OLD_KEYS = ["centered", "clipped", "norm2", "replaced", "scale", "tau"]
NEW_KEYS = ["noise_multiplier", "seed", "sequence", "sigma"]


@pytest.fixture(scope="module")
def keys():
    return list(Golden("avg_lenet5_n10").clients()[0])


@pytest.fixture(scope="module")
def g0(keys):
    lenet = Golden("avg_lenet5_n10").clients()
    return {k: _host(lenet[0][k]).astype(np.float32) for k in keys}


@pytest.fixture(scope="module")
def clients(g0, keys):
    cl = make_round(g0, 1, keys)
    cl[3] = {k: np.full_like(v, np.nan) for k, v in cl[3].items()}  # one poisoned upload
    return cl


@pytest.fixture(scope="module")
def tau(g0, keys):
    norms = norms_of(make_round(g0, 1, keys), g0, keys)  # growing with the client index
    return float(0.5 * (norms[5] + norms[6]))  # clients 6..9 scaled, client 3 replaced: 5 with s < 1


def noised_reference(engine, clients, centre, tau, mult, seed, sequence, extra=None, fp32_out=False):
    """{key: (want, bound)} for the fp32 keys, by the derivation above; checks the audit on the way."""
    audit = engine.last_clip
    assert sorted(audit) == sorted(OLD_KEYS + NEW_KEYS)
    sigma = float(np.float32(mult * tau))
    assert (audit["noise_multiplier"], audit["sigma"], audit["seed"], audit["sequence"]) == (mult, sigma, seed, sequence)
    scale = clip.clip_scales(audit["norm2"], tau)
    assert audit["tau"] == tau and audit["scale"].tobytes() == scale.tobytes() and audit["centered"] is True
    n = len(clients)
    out = {}
    for s in engine.last_plan.groups["f32"].segments:
        if s.numel == 0:
            continue
        x = np.stack([_host(c[s.key]).astype(np.float32).reshape(-1) for c in clients])
        g = _host(centre[s.key]).astype(np.float32).reshape(-1)
        total = cr.clipped_sum(x, g, scale).astype(np.float64)
        z = nr.normals(seed, sequence, s.offset, s.numel)  # the key's absolute columns of the bucket row
        zz = np.abs(z) + nr.Z_ERROR
        want = (total + sigma * z) / n
        bound = (sigma * nr.Z_ERROR + U * sigma * zz + 2.0 ** -150 + U * (np.abs(total) + sigma * zz * (1 + U) + 2.0 ** -150)) / n
        bound = bound * (1 + 2.0 ** -52) + np.abs(want) * 2.0 ** -53
        if extra is not None:  # FedAVGM's first step: two float64 roundings
            bound = bound + 2 * 2.0 ** -53 * (np.abs(want) + bound + np.abs(g))
        if fp32_out:
            bound = bound + U * (np.abs(want) + bound)
        shape = _host(clients[0][s.key]).shape
        out[s.key] = (want.reshape(shape), bound.reshape(shape), (sigma * z / n).reshape(shape))
    return scale, out


def check(got, ref, where):
    worst = 0.0
    for k, (want, bound, _) in ref.items():
        err = np.abs(_host(got[k]).astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"{where}: {k}: error {err.max():.3g}, bound {bound.max():.3g}"
    print(f"{where}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("output", OUTPUTS)
def test_no_noise_is_the_parents_round(output, clients, g0, tau, cuda):
    plain = NormClip(tau=tau, output=output)
    plain.init_global(g0)
    want = plain.server(upload(clients), 0)["w_glob"]
    audit = plain.engine.last_clip
    assert sorted(audit) == OLD_KEYS  # a round not asked for noise keeps the parent's audit
    assert audit["replaced"].tolist() == [3] and audit["clipped"].tolist() == [3, 6, 7, 8, 9]
    for mult in (0, 0.0):
        s = NormClip(tau=tau, output=output, noise_multiplier=mult, seed=SEED, sequence=9)
        s.init_global(g0)
        same(s.server(upload(clients), 0)["w_glob"], want, f"multiplier {mult!r} {output}")
        got = s.engine.last_clip
        assert sorted(got) == sorted(OLD_KEYS + NEW_KEYS) and all(got[k] is None for k in NEW_KEYS)
        for k in OLD_KEYS:
            assert np.asarray(got[k]).tobytes() == np.asarray(audit[k]).tobytes(), k  # (a NaN norm included)
        assert s.sequence == 9  # no noise was added: the sequence stays


@pytest.mark.parametrize("output", OUTPUTS)
def test_noised_round_matches_the_reference(output, clients, g0, keys, tau, cuda):
    mult = 1.25
    s = NormClip(tau=tau, output=output, noise_multiplier=mult, seed=SEED)
    s.init_global(g0)
    got = s.server(upload(clients), 0)["w_glob"]
    scale, ref = noised_reference(s.engine, clients, g0, tau, mult, SEED, 0, fp32_out=output != "reference")
    assert int((scale < 1).sum()) == 5 and int((scale == 0).sum()) == 1
    assert all(np.isfinite(_host(v)).all() for v in got.values())
    check(got, ref, f"noised {output}")
    if output == "reference":
        # the noise is there: the mean moved by about sigma / N per column, far beyond the bound
        plain = NormClip(tau=tau)
        plain.init_global(g0)
        base = plain.server(upload(clients), 0)["w_glob"]
        moved = np.concatenate([(_host(got[k]) - _host(base[k])).reshape(-1) for k in keys])
        noise = np.concatenate([ref[k][2].reshape(-1) for k in keys])
        assert np.abs(moved - noise).max() <= 2 * max(b.max() for _, b, _ in ref.values())
        assert abs(moved.std() / (s.engine.last_clip["sigma"] / N) - 1) < 0.05


def test_fused_avgm_step(clients, g0, keys, tau, cuda):
    mult = 0.75
    opt = ServerOptimizer("avgm")
    opt.init_global(g0)
    s = NormClip(tau=tau, server_opt=opt, noise_multiplier=mult, seed=SEED, sequence=5)
    s.init_global(g0)
    got = s.server(upload(clients), 0)["w_glob"]
    _, ref = noised_reference(s.engine, clients, g0, tau, mult, SEED, 5, extra="avgm")
    check(got, ref, "fused AVGM")  # v = 0: w = l + (g - l)
    assert s.sequence == 6


def test_two_rounds_and_a_restart(clients, g0, keys, tau, cuda):
    mult = 1.0

    def run(strategy):
        first = strategy.server(upload(clients), 0)["w_glob"]
        a0 = dict(strategy.engine.last_clip)
        centre = {k: np.asarray(first[k]).astype(np.float32) for k in keys}  # what the strategy subtracts next
        cl2 = make_round(centre, 8, keys)
        second = strategy.server(upload(cl2), 1)["w_glob"]
        return first, a0, centre, cl2, second, dict(strategy.engine.last_clip)

    s = NormClip(tau=tau, noise_multiplier=mult, seed=SEED)
    s.init_global(g0)
    first, a0, centre, cl2, second, a1 = run(s)
    assert (a0["sequence"], a1["sequence"], s.sequence) == (0, 1, 2) and a0["seed"] == a1["seed"] == SEED
    _, ref2 = noised_reference(s.engine, cl2, centre, tau, mult, SEED, 1)
    check(second, ref2, "second round")
    k = keys[0]
    off = next(seg.offset for seg in s.engine.last_plan.groups["f32"].segments if seg.key == k)
    z0, z1 = (nr.normals(SEED, q, off, g0[k].size) for q in (0, 1))
    assert not np.isclose(z0, z1).any()  # another sequence: other noise, which `check` has just held round 1 to
    t = NormClip(tau=tau, noise_multiplier=mult, seed=SEED)  # the same seed from sequence 0: the same rounds
    t.init_global(g0)
    first_t, _, _, _, second_t, _ = run(t)
    same(first_t, first, "restart, round 0")
    same(second_t, second, "restart, round 1")
    r = NormClip(tau=tau, noise_multiplier=mult, seed=SEED, sequence=1)  # resumed at the next sequence
    r.init_global(centre)
    same(r.server(upload(cl2), 1)["w_glob"], second, "resumed at sequence 1")
    other = NormClip(tau=tau, noise_multiplier=mult, seed=SEED + 1)
    other.init_global(g0)
    assert not rr.same_bits(_host(other.server(upload(clients), 0)["w_glob"][k]), _host(first[k]))


def test_a_noised_first_round_without_init_global_is_refused(clients, tau, cuda):
    s = NormClip(tau=tau, noise_multiplier=1.0, seed=SEED)
    with pytest.raises(SystemExit):
        s.server(upload(clients), 0)
    assert s.sequence == 0 and s._prev_glob is None
    with pytest.raises(ValueError, match="centre"):
        s.engine.ensemble_clipped(clients, tau, None, center=None, noise_multiplier=1.0, seed=SEED)


def test_bn_counters_are_not_noised(cuda):
    bn = Golden("avg_bnmodel_pyint_n4").clients()
    names = list(bn[0])
    rng = np.random.default_rng(5)
    base = {k: _host(bn[0][k]) for k in names}
    cl = []
    for i in range(7):
        c = {}
        for k in names:
            v = base[k]
            if v.dtype == np.float32:
                c[k] = (v + np.float32(0.05 * (i + 1)) * rng.standard_normal(v.shape).astype(np.float32)).astype(np.float32)
            else:
                c[k] = (v + v.dtype.type(10 * i + 1)).astype(v.dtype)
        cl.append(c)
    tau = float(np.sort(norms_of(cl, base, f32_keys(base)))[3])
    plain = NormClip(tau=tau)
    plain.init_global(base)
    want = plain.server(upload(cl), 0)["w_glob"]
    s = NormClip(tau=tau, noise_multiplier=2.0, seed=SEED)
    s.init_global(base)
    got = s.server(upload(cl), 0)["w_glob"]
    assert list(got) == list(want)
    others = [k for k in names if base[k].dtype != np.float32]
    assert others and any(k.endswith("num_batches_tracked") for k in others)
    for k in names:
        if k in others:  # int64 / float64 buffers: outside the guarantee, untouched by the noise
            assert rr.same_bits(_host(got[k]), _host(want[k])), k
        elif base[k].size > 1:
            assert not rr.same_bits(_host(got[k]), _host(want[k])), k
    _, ref = noised_reference(s.engine, cl, base, tau, 2.0, SEED, 0)
    check(got, ref, "bn model")
