"""The stripe and shard planner of the multi-GPU aggregation: pure arithmetic (no tensors, no process group, no GPU).
The column layout a ShardPlan describes is in flearn_amd.dist's docstring; the stripe widths come from a two-stage
pipeline model (`StripeModel`), whose coefficients bench.py fits on the running job before it plans.
"""
from __future__ import annotations

from dataclasses import dataclass

ALIGN = 64


def round_up(x: int, m: int = ALIGN) -> int:
    """x rounded up to a multiple of m."""
    return -(-x // m) * m


def cols_per_rank(n_cols: int, world: int) -> int:
    """Columns each of `world` ranks holds of an n_cols bucket (not yet rounded to ALIGN)."""
    return -(-max(n_cols, 1) // max(world, 1))


@dataclass(frozen=True)
class StripeModel:
    """Per-stripe cost model of one rank (seconds; widths in columns per rank). reduce(S) = a_r + b_r*S on the compute
    stream; gather(S) = a_g + b_g*S on the collective's stream (a stripe of S columns per rank is an all-gather of
    world*S columns).  Contention: a reduce that runs beside a gather streams (1 + c_r) times slower, a gather that
    runs beside a reduce (1 + c_g) times slower — they share the CUs and the HBM.  Measured on one MI355X with a copy
    kernel standing in for the gather (tools/overlap_probe.py); 0 = the optimistic model (perfect
    overlap)."""

    a_r: float
    b_r: float
    a_g: float
    b_g: float
    c_r: float = 0.0
    c_g: float = 0.0

    @staticmethod
    def assumed(n_clients: int, world: int, hbm_bytes_s: float = 7.0e12, link_bytes_s: float = 50e9,
                launch_s: float = 10e-6, collective_s: float = 30e-6) -> "StripeModel":
        """A priori coefficients: the reduce streams N*4 B per column at the measured 1-GPU rate (~7 TB/s);
        an all-gather brings (world-1)*4 B per column into each GPU over its world-1 xGMI links (one per peer on an
        MI355X node) at an assumed per-link rate. bench.py replaces them with measured ones."""
        ingress = max(world - 1, 1) * link_bytes_s
        return StripeModel(launch_s, n_clients * 4.0 / hbm_bytes_s, collective_s,
                           max(world - 1, 0) * 4.0 / ingress)

    @staticmethod
    def fit(w_big: int, w_small: int, r_big: float, r_small: float, g_big: float, g_small: float,
            c_r: float = 0.0, c_g: float = 0.0) -> "StripeModel":
        """Coefficients from two widths' measured reduce and gather times (non-negative), plus the contention terms
        (measured separately)."""
        def line(tb, ts):
            b = max((tb - ts) / max(w_big - w_small, 1), 0.0)
            return max(ts - b * w_small, 0.0), b

        a_r, b_r = line(r_big, r_small)
        a_g, b_g = line(g_big, g_small)
        return StripeModel(a_r, b_r, a_g, b_g, max(c_r, 0.0), max(c_g, 0.0))

    def with_contention(self, c_r: float, c_g: float) -> "StripeModel":
        return StripeModel(self.a_r, self.b_r, self.a_g, self.b_g, max(c_r, 0.0), max(c_g, 0.0))

    def makespan(self, widths, rep: int = 0) -> tuple:
        """(step time, reduce-stream busy time, exposed gather time) of a stripe plan; `rep` replicated columns are
        reduced after the stripes, with no gather.  Every stripe's reduce but the first runs beside the previous
        stripe's gather, and every gather but one that finds the reduce stream idle runs beside a reduce: those
        streaming terms carry the contention factors (1 + c_r) and (1 + c_g)."""
        t_red = t_gat = 0.0
        last = len(widths) - 1
        for c, w in enumerate(widths):
            t_red += self.a_r + self.b_r * w * (1.0 + (self.c_r if c > 0 else 0.0))
            busy_after = c < last or rep > 0  # a reduce (next stripe or the tail) runs beside it
            t_gat = max(t_red, t_gat) + self.a_g + self.b_g * w * (1.0 + (self.c_g if busy_after else 0.0))
        if rep:
            t_red += self.a_r + self.b_r * rep * (1.0 + (self.c_r if widths else 0.0))
        step = max(t_gat, t_red)
        return step, t_red, step - t_red


def plan_stripes(local_cols: int, model: StripeModel, max_stripes: int = 8, rep: int = 0) -> tuple:
    """Stripe widths (multiples of ALIGN summing to >= local_cols) minimising the model's makespan (followed by `rep`
    replicated columns).  Candidates: k = 1..max_stripes stripes with geometric widths S_c ~ q**c for q on a grid (q <
    1: big stripes first, the usual choice when the reduce dominates; q > 1: a small first stripe so the gathers start
    early, when the collective dominates)."""
    units = max(1, round_up(local_cols) // ALIGN)
    best = ((units * ALIGN,), model.makespan((units * ALIGN,), rep)[0])
    for k in range(2, min(max_stripes, units) + 1):
        for q in (0.125, 0.25, 0.35, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.15, 1.3, 1.5, 2.0, 3.0, 4.0):
            raw = [q**c for c in range(k)]
            tot = sum(raw)
            u = [max(1, int(units * x / tot)) for x in raw]
            u[0 if q <= 1 else -1] += units - sum(u)  # the remainder goes to the big end
            if min(u) < 1:
                continue
            widths = tuple(x * ALIGN for x in u)
            t = model.makespan(widths, rep)[0]
            if t < best[1] - 1e-12:
                best = (widths, t)
    return best[0]


def _plan_with_tail(n_cols: int, world: int, covered: int, model: StripeModel, max_stripes: int):
    """(stripe widths, rep) of the best plan whose stripes cover the largest multiple of world*ALIGN within `covered`
    columns, the other `rep` being the replicated tail; None if either is empty."""
    units = covered // (world * ALIGN)
    rep = n_cols - world * units * ALIGN
    if units < 1 or rep <= 0:
        return None
    return plan_stripes(units * ALIGN, model, max_stripes, rep=rep), rep


#: replicated-tail sizes plan_shards tries, as fractions of the bucket
REP_FRACTIONS = (0.0, 0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.125, 0.15, 0.175, 0.2, 0.25, 0.3, 0.35, 0.4,
                 0.45, 0.5, 0.55, 0.6)


def plan_shards(n_cols: int, world: int, model: StripeModel, max_stripes: int = 8,
                fractions=REP_FRACTIONS) -> tuple:
    """(stripe widths, replicated tail columns) minimising the model's makespan for an n_cols bucket on `world` ranks:
    the padded plan with no tail, against plans whose stripes cover exactly world*sum(widths) = n_cols - rep columns
    and whose last `rep` columns every rank reduces itself (ShardPlan.rep).  A tail pays where the gather dominates:
    each replicated column costs every rank one column of reduce and saves (world-1)/world of a column of gather
    ingress."""
    w0 = plan_stripes(cols_per_rank(n_cols, world), model, max_stripes)
    best = (w0, 0, model.makespan(w0)[0])
    if world < 2:
        return best[0], 0
    for f in fractions:
        cand = _plan_with_tail(n_cols, world, int(n_cols * (1.0 - f)), model, max_stripes)
        if cand is None:
            continue
        t = model.makespan(*cand)[0]
        if t < best[2] - 1e-12:
            best = (*cand, t)
    return best[0], best[1]


#: the reduce's and a concurrent all-gather stand-in's slowdowns measured on one MI355X
#: (tools/overlap_probe.py, profiles/r04/overlap/: a 32-64-block copy at 0.3-0.55 TB/s beside the
#: default-grid reduce) — the prior for the contended candidate plans
CONTENTION_PRIOR = (0.37, 0.82)


def shard_candidates(n_cols: int, world: int, model: StripeModel, max_stripes: int = 8,
                     contention=CONTENTION_PRIOR) -> list:
    """The plans a measured trial chooses among (bench.py times each for a few steps on the running job): plan_shards'
    best, the best plan with no replicated tail, and the best with half and with 1.5x the best's tail; then the best
    plan of the same model with the measured one-GPU contention terms (RCCL's kernels and the reduce share CUs and
    HBM: a concurrent gather slows the reduce by ~1/3 and itself ~1.8x, profiles/r04/overlap/) and the plain serial
    plan — one stripe, no overlap at all.  The model's overlap is the optimistic end; the measured step picks."""
    best = plan_shards(n_cols, world, model, max_stripes)
    out = [best]
    if world < 2:
        return out
    lc = cols_per_rank(n_cols, world)
    cands = [(plan_stripes(lc, model, max_stripes), 0)]
    if best[1] >= 4 * world * ALIGN:
        for rep_target in (best[1] // 2, min(int(best[1] * 1.5), int(n_cols * 0.75))):
            cands.append(_plan_with_tail(n_cols, world, int(n_cols - rep_target), model, max_stripes))
    if contention is not None and (model.c_r, model.c_g) == (0.0, 0.0):
        cands.append(plan_shards(n_cols, world, model.with_contention(*contention), max_stripes))
    cands.append(((round_up(lc),), 0))  # serial: reduce everything, then one gather
    for c in cands:
        if c is not None and c not in out:
            out.append(c)
    return out


@dataclass(frozen=True)
class ShardPlan:
    n_cols: int  # real global columns (parameters)
    world: int
    rank: int
    widths: tuple  # S_c: columns per (stripe c, rank) slice, each a multiple of ALIGN
    rep: int = 0  # replicated tail: global columns [n_cols - rep, n_cols), reduced by every rank

    @staticmethod
    def make(n_cols: int, world: int, rank: int, stripes: int = 4, weights=None) -> "ShardPlan":
        """Equal stripes by default; `weights` (one per stripe) sizes them unevenly, e.g. (3, 1): the gather of the
        big first stripe hides behind the small last stripe's reduce and only the last stripe's gather stays
        exposed."""
        if world < 1 or not 0 <= rank < world or stripes < 1:
            raise ValueError("bad world / rank / stripes")
        if weights is None:
            return ShardPlan(n_cols, world, rank, (round_up(cols_per_rank(n_cols, world * stripes)),) * stripes)
        weights = tuple(float(x) for x in weights)
        if len(weights) != stripes or min(weights) <= 0:
            raise ValueError("need one positive weight per stripe")
        if stripes == 1:
            return ShardPlan.make(n_cols, world, rank, 1)
        total = round_up(cols_per_rank(n_cols, world))
        widths, acc = [], 0
        for c in range(stripes - 1):
            w = round_up(int(total * weights[c] / sum(weights)))
            w = max(ALIGN, min(w, total - acc - ALIGN * (stripes - 1 - c)))
            widths.append(w)
            acc += w
        widths.append(max(ALIGN, total - acc))
        return ShardPlan(n_cols, world, rank, tuple(widths))

    @staticmethod
    def from_widths(n_cols: int, world: int, rank: int, widths, rep: int = 0) -> "ShardPlan":
        """A plan with explicit per-rank stripe widths (e.g. from plan_stripes / plan_shards); rep > 0: the stripes
        cover exactly the first n_cols - rep columns (no padding) and every rank reduces the last rep itself."""
        widths = tuple(int(w) for w in widths)
        rep = int(rep)
        if not widths or any(w <= 0 or w % ALIGN for w in widths):
            raise ValueError("stripe widths must be positive multiples of ALIGN")
        if rep < 0 or (rep and world * sum(widths) + rep != n_cols):
            raise ValueError("a replicated tail needs stripes covering exactly n_cols - rep columns")
        if world * sum(widths) + rep < n_cols:
            raise ValueError("stripes do not cover the bucket")
        if world < 1 or not 0 <= rank < world:
            raise ValueError("bad world / rank")
        return ShardPlan(n_cols, world, rank, widths, rep)

    @property
    def stripes(self) -> int:
        return len(self.widths)

    @property
    def shard(self) -> int:
        """The slice width when all stripes are equal."""
        if len(set(self.widths)) != 1:
            raise ValueError("stripes differ in width: use shard_of(stripe)")
        return self.widths[0]

    def shard_of(self, stripe: int) -> int:
        return self.widths[stripe]

    @property
    def padded(self) -> int:
        """Global columns the stripes cover (the gathered range; padding included when rep == 0)."""
        return self.world * sum(self.widths)

    @property
    def full_cols(self) -> int:
        """Columns of the reassembled bucket: the gathered range and the replicated tail."""
        return self.padded + self.rep

    @property
    def local_stripes(self) -> int:
        """Local columns of the stripes (the tail's local columns follow them)."""
        return sum(self.widths)

    @property
    def local_cols(self) -> int:
        return sum(self.widths) + self.rep

    @property
    def local_stride(self) -> int:
        """Row stride of the rank's local stack and state (local_cols rounded up to ALIGN, so every row stays 16-B
        aligned whatever the tail's width)."""
        return round_up(self.local_cols)

    def segments(self):
        """(local begin, global begin, width) of every local column range: the stripes, then the replicated tail."""
        out = [(self.local_begin(c), self.global_begin(c), self.widths[c]) for c in range(self.stripes)]
        if self.rep:
            out.append((self.local_stripes, self.padded, self.rep))
        return out

    def local_begin(self, stripe: int) -> int:
        return sum(self.widths[:stripe])

    def global_begin(self, stripe: int, rank: int | None = None) -> int:
        r = self.rank if rank is None else rank
        return self.world * self.local_begin(stripe) + r * self.widths[stripe]

    def local_to_global(self, local_col: int) -> int:
        for lo, g0, w in self.segments():
            if lo <= local_col < lo + w:
                return g0 + (local_col - lo)
        raise IndexError(local_col)

    def real_cols_in_slice(self, stripe: int, rank: int | None = None) -> int:
        """Columns of this slice that are real parameters (the tail slices may be padding)."""
        g0 = self.global_begin(stripe, rank)
        return max(0, min(self.widths[stripe], self.n_cols - g0))
