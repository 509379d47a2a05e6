"""Robust aggregation on the MI355X engine: the coordinate-wise trimmed mean and median of Yin et
al. (ICML 2018), and Krum / multi-Krum of Blanchard et al. (NeurIPS 2017), which judges whole uploads
(below).  flearn has no counterpart; all take FedAVG's place (avg.py:11-46), with its
`client` / `client_receive` and upload format.

Per model element the N clients' values are ordered (IEEE totalOrder, so NaN and inf have a place),
the `trim` smallest and largest are dropped and the rest are averaged: up to `trim` uploads per
side that are NaN, inf or scaled leave every element of the global model finite, where one such
upload poisons FedAVG's weighted mean.  `agg_weight` must be present in each upload, as in
flearn's upload format, and is NOT used: a client must not be able to buy influence with its own
weight.  The result does not depend on the order of the uploads.
"""
from __future__ import annotations

import math
import secrets

import numpy as np
import torch

from .avg import AVG
from .strategy import StrategyRound


class _RobustRound(AVG):
    """What the robust strategies share: FedAVG's client side, every client at once, and an optional
    ServerOptimizer (`server_opt`, set by the subclass) fused into the round's divide."""

    server_opt = None

    def server(self, ensemble_params_lst, round_):
        """{"w_glob": the robust round's result (server_ensemble: the trimmed mean, or the mean of the
        selected uploads)}; client-data errors -> server_exception, device errors propagate."""
        return {"w_glob": self._ensemble_or_exit(ensemble_params_lst, server_opt=self.server_opt)}

    def begin_round(self, round_):
        raise ValueError("a robust round needs every client at once: begin_round() is not supported")


class TrimmedMean(_RobustRound):
    """Coordinate-wise trimmed mean.  trim: a float in [0, 0.5) is the fraction dropped per side,
    t = floor(trim * N) each round; an int is the count per side (0 <= 2 t < N is checked per
    round).  trim = 0 is a mean summed in sorted order, not FedAVG's list-order sum.
    server_opt: a ServerOptimizer (AVGM / Adagrad / Yogi / Adam) fused into the round's divide,
    with w_local := the previous global model, as AVGM / OPT(server_side=True) do.
    At most 128 clients per round, one device, fp32 / float64 / int64 tensors; anything else takes
    server_exception's route, like any client-data error.  `agg_weight` is required and ignored."""

    def __init__(self, trim=0.1, server_opt=None, encrypt=None, output="reference", device=None, devices=None,
                 group=None, chunk_clients=None):
        super().__init__(encrypt, output, device, devices, group, chunk_clients)
        self.trim = self._check_trim(trim)
        self.server_opt = server_opt

    @staticmethod
    def _check_trim(trim):
        if isinstance(trim, (bool, np.bool_)):
            raise ValueError("trim must be a fraction in [0, 0.5) or a count >= 0, not a bool")
        if isinstance(trim, (int, np.integer)):
            if trim < 0:
                raise ValueError(f"trim count must be >= 0, got {trim}")
            return int(trim)
        if isinstance(trim, (float, np.floating)):
            if not 0.0 <= trim < 0.5:  # NaN fails both
                raise ValueError(f"trim fraction must be in [0, 0.5), got {trim}")
            return float(trim)
        raise ValueError(f"trim must be a float fraction or an int count, got {type(trim).__name__}")

    def trim_count(self, n_clients: int) -> int:
        """Values dropped per side in a round of n_clients uploads."""
        if isinstance(self.trim, float):
            return math.floor(self.trim * n_clients)
        return self.trim

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        """The engine's robust round (Aggregator.ensemble_trimmed).  agg_weight_lst is checked for
        presence by server_pre_processing and not used."""
        return self.engine.ensemble_trimmed(w_local_lst, self.trim_count(len(w_local_lst)), key_lst, server_opt=server_opt)


class Median(TrimmedMean):
    """Coordinate-wise median: the trimmed mean with t = (N - 1) // 2, which keeps one value for
    odd N and the mean of the two middle values for even N.  `agg_weight` is required and ignored."""

    def __init__(self, server_opt=None, encrypt=None, output="reference", device=None, devices=None, group=None,
                 chunk_clients=None):
        super().__init__(0, server_opt, encrypt, output, device, devices, group, chunk_clients)

    def trim_count(self, n_clients: int) -> int:
        return max(0, (n_clients - 1) // 2)


class MultiKrum(_RobustRound):
    """Multi-Krum (Blanchard et al., NeurIPS 2017): with up to f bad uploads among N, an upload's
    score is the sum of its squared distances to its N - f - 2 nearest other uploads; the m uploads
    of lowest score are averaged with equal weights and the others are left out whole.  The engine's
    audit of a round is `self.engine.last_krum` ("selected": who was kept, in upload order).
    f: ints only, N >= 2 f + 3 is checked per round; m: None = N - f per round, else 1 <= m <= N - f.
    center: "previous" (the default) subtracts this strategy's own last w_glob (a copy it keeps) from
    every upload before the distances are taken — models of one round are g + delta with
    |delta| << |g|, and G_ii + G_jj - 2 G_ij of uncentred rows cancels to a few digits, while
    fl32(x - g) is nearly exact and distances do not depend on the centre; the first round runs
    uncentred.  None never centres.  The centre is the server's own state, never a client's row.
    server_opt: a ServerOptimizer fused into the divide, as for TrimmedMean.  Distances are measured
    on the fp32 tensors only (int64 / float64 buffers such as BN counters do not enter them).  At
    most 128 clients per round, one device; more than f non-finite uploads, like any client-data
    error, take server_exception's route.  `agg_weight` is required and ignored: a client must not be
    able to buy influence with its own weight."""

    def __init__(self, f, m=None, server_opt=None, center="previous", encrypt=None, output="reference", device=None,
                 devices=None, group=None, chunk_clients=None):
        super().__init__(encrypt, output, device, devices, group, chunk_clients)
        self.f = self._check_count("f", f, 0)
        self.m = None if m is None else self._check_count("m", m, 1)
        if center is not None and center != "previous":
            raise ValueError(f'center must be "previous" or None, got {center!r}')
        self.center = center
        self.server_opt = server_opt
        self._prev_glob = None

    @staticmethod
    def _check_count(name, v, lo):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
        return int(v)

    def select_count(self, n_clients: int) -> int:
        """Uploads averaged in a round of n_clients."""
        return n_clients - self.f if self.m is None else self.m

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        """The engine's Krum round (Aggregator.ensemble_krum).  agg_weight_lst is checked for presence
        by server_pre_processing and not used."""
        center = self._prev_glob if self.center == "previous" else None
        w_glob = self.engine.ensemble_krum(w_local_lst, self.f, self.select_count(len(w_local_lst)), key_lst,
                                           server_opt=server_opt, center=center)
        if self.center == "previous":  # a copy of its own: the caller may change what it is handed
            self._prev_glob = {k: v.detach().clone() if isinstance(v, torch.Tensor) else np.array(v)
                               for k, v in w_glob.items()}
        return w_glob


class Krum(MultiKrum):
    """Krum: the one upload of lowest score becomes the global model (MultiKrum with m = 1).
    `agg_weight` is required and ignored."""

    def __init__(self, f, server_opt=None, center="previous", encrypt=None, output="reference", device=None,
                 devices=None, group=None, chunk_clients=None):
        super().__init__(f, 1, server_opt, center, encrypt, output, device, devices, group, chunk_clients)


class NormClip(_RobustRound):
    """Norm clipping (Sun et al. 2019; the clipping step of McMahan et al. 2018): every client's update
    x_i - g is projected onto the ball of radius tau around the server's model g, then the uploads are
    averaged with equal weights.  No upload is left out, no bound on the number of attackers is needed
    and two clients are enough: a scaled or boosted upload keeps its direction and loses its leverage,
    and a NaN / inf upload counts as a zero update.  The engine's audit of a round is
    `self.engine.last_clip` ("norm2", "scale", "tau", "clipped", "replaced", "centered").
    Exactly one of tau (a float > 0, inf allowed) and quantile (q in (0, 1]: each round's radius is the
    ceil(q * F)-th smallest of the F finite client norms, Andrew et al. 2021) is given.
    center: "previous" — g is this strategy's own last w_glob (a copy it keeps); `init_global(w_glob)`
    sets the first one.  Without it the FIRST ROUND IS UNDEFENDED: it is the plain unit-weight mean,
    there being nothing to measure updates against.  center=None is refused: clipping needs a centre.
    server_opt: a ServerOptimizer fused into the divide, as for TrimmedMean.  Norms are measured on the
    fp32 tensors only (int64 / float64 buffers such as BN counters do not enter them and are averaged
    over all clients).  At most 128 clients per round, one device; client-data errors take
    server_exception's route.  `agg_weight` is required and ignored: a client must not be able to buy
    influence with its own weight.

    noise_multiplier > 0 (keyword-only, with a fixed tau) makes every round DP-FedAvg's (McMahan et al.
    2018): Gaussian noise of standard deviation noise_multiplier * tau is added on the device to the
    SUM of the clipped uploads, so the mean's is noise_multiplier * tau / N; `last_clip` then also
    carries "noise_multiplier", "sigma", "seed" and "sequence".  The noise is a function of (seed,
    sequence, column): seed=None draws secrets.randbits(64) at construction (`self.seed`), and
    `self.sequence` advances by one per noised round.  REUSING A (seed, sequence) PAIR REPEATS THE
    NOISE: a caller that restarts with an explicit seed must pass the next sequence.  Noise is refused
    with quantile=, with tau = inf, and on a first round without `init_global` (which would run
    unclipped).  The engine adds the noise and nothing else: the accounting of (epsilon, delta) and the
    sampling of clients are the caller's, float64 / int64 buffers are not noised, and Philox is a
    statistical generator, not a cryptographic one."""

    def __init__(self, tau=None, quantile=None, server_opt=None, center="previous", encrypt=None, output="reference",
                 device=None, devices=None, group=None, chunk_clients=None, *, noise_multiplier=None, seed=None,
                 sequence=0):
        from .. import clip

        super().__init__(encrypt, output, device, devices, group, chunk_clients)
        self.tau, self.quantile = clip.check_radius(tau, quantile)
        if center != "previous":
            raise ValueError(f'center must be "previous" (clipping needs a centre), got {center!r}')
        self.center = center
        self.server_opt = server_opt
        self._prev_glob = None
        self.noise_multiplier = noise_multiplier
        self.seed = secrets.randbits(64) if seed is None else seed
        self.sequence = sequence
        # the multiplier, and with noise on the radius, the seed and the sequence, refused here as the
        # round would refuse them
        self._noised = clip.check_noise(noise_multiplier, self.seed, sequence, self.tau, self.quantile, True) is not None

    @staticmethod
    def _copy(w_glob):
        return {k: v.detach().clone() if isinstance(v, torch.Tensor) else np.array(v) for k, v in w_glob.items()}

    def init_global(self, w_glob):
        """The model the first round's updates are measured against (a copy is kept)."""
        if not hasattr(w_glob, "keys"):
            raise ValueError("init_global takes a w_glob-like dict")
        self._prev_glob = self._copy(w_glob)

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        """The engine's clipped round (Aggregator.ensemble_clipped).  agg_weight_lst is checked for
        presence by server_pre_processing and not used."""
        w_glob = self.engine.ensemble_clipped(w_local_lst, self.tau, self.quantile, key_lst, server_opt=server_opt,
                                              center=self._prev_glob, noise_multiplier=self.noise_multiplier,
                                              seed=self.seed, sequence=self.sequence)
        if self._noised:  # the round added its noise: never this (seed, sequence) again
            self.sequence += 1
        self._prev_glob = self._copy(w_glob)  # a copy of its own: the caller may change what it is handed
        return w_glob


class StreamedNormClip(AVG):
    """NormClip for any number of clients: the clipped (noise_multiplier: DP-FedAvg) round aggregated
    in chunks of chunk_clients <= 128 clients (Aggregator.ensemble_clipped_chunked /
    begin_clipped_round), with device memory O(chunk_clients x model) whatever the client count, and
    bit-identical to NormClip(tau=...) on the rounds NormClip takes.  `server(uploads, round_)` takes the
    whole list; `begin_round(round_)` returns a handle whose `add(upload | encoded str)` aggregates
    uploads as they arrive and whose `finish()` returns what server() returns.  The engine's audit of
    a round is `self.engine.last_clip` (NormClip's keys, the arrays over all clients in list order,
    and "chunks").

    Limits: a FIXED tau only (a streamed round cannot know a quantile of norms it has not seen), unit
    weights (`agg_weight` is required and ignored), one device.  center, `init_global`, the undefended
    first round without it, server_opt, noise_multiplier, seed and sequence are NormClip's:
    seed=None draws secrets.randbits(64), `self.sequence` advances by one per noised round (at
    finish()), and REUSING A (seed, sequence) PAIR REPEATS THE NOISE."""

    def __init__(self, tau, server_opt=None, center="previous", encrypt=None, output="reference", device=None,
                 chunk_clients=16, *, noise_multiplier=None, seed=None, sequence=0):
        from .. import _native as na
        from .. import clip

        if (isinstance(chunk_clients, (bool, np.bool_)) or not isinstance(chunk_clients, (int, np.integer))
                or not 1 <= chunk_clients <= na.CLIP_MAX_CLIENTS):
            raise ValueError(f"chunk_clients must be an int in [1, {na.CLIP_MAX_CLIENTS}], got {chunk_clients!r}")
        super().__init__(encrypt, output, device, None, None, int(chunk_clients))
        self.tau, _ = clip.check_radius(tau, None)
        if center != "previous":
            raise ValueError(f'center must be "previous" (clipping needs a centre), got {center!r}')
        self.center = center
        self.server_opt = server_opt
        self._prev_glob = None
        self.noise_multiplier = noise_multiplier
        self.seed = secrets.randbits(64) if seed is None else seed
        self.sequence = sequence
        self._noised = clip.check_noise(noise_multiplier, self.seed, sequence, self.tau, None, True) is not None

    _copy = staticmethod(NormClip._copy)
    init_global = NormClip.init_global

    def _clip_args(self) -> dict:
        return dict(center=self._prev_glob, chunk_clients=self.chunk_clients, noise_multiplier=self.noise_multiplier,
                    seed=self.seed, sequence=self.sequence)

    def _after_round(self, w_glob):
        if self._noised:  # the round added its noise: never this (seed, sequence) again
            self.sequence += 1
        self._prev_glob = self._copy(w_glob)  # a copy of its own: the caller may change what it is handed
        return w_glob

    def server(self, ensemble_params_lst, round_):
        """{"w_glob": the streamed clipped round's result}; client-data errors -> server_exception,
        device errors propagate."""
        return {"w_glob": self._ensemble_or_exit(ensemble_params_lst, server_opt=self.server_opt)}

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        """The engine's streamed clipped round (Aggregator.ensemble_clipped_chunked).  agg_weight_lst is
        checked for presence by server_pre_processing and not used."""
        return self._after_round(self.engine.ensemble_clipped_chunked(w_local_lst, self.tau, key_lst,
                                                                      server_opt=server_opt, **self._clip_args()))

    def _round_done(self, w_glob, uploads):
        return {"w_glob": self._after_round(w_glob)}

    def begin_round(self, round_):
        return _StreamedClipRound(self, round_)


class _StreamedClipRound(StrategyRound):
    """StreamedNormClip.begin_round's handle: StrategyRound over the engine's ClippedRoundAccumulator."""

    def _begin(self, first_params):
        s = self.strategy
        self._acc = self._guard(lambda: s.engine.begin_clipped_round(s.tau, key_lst=None, server_opt=s.server_opt,
                                                                     **s._clip_args()))
