"""Strategy registry — flearn/common/utils.py:12-58 (`setup_strategy`, `base_strategy_lst`)."""
from __future__ import annotations

import random

import numpy as np
import torch

from .strategy import AVG, AVGM, BN, LG, LG_R, OPT, SGD, Distill, Dyn, Krum, Median, MultiKrum, NormClip, Prox, QuantizedAVG, StreamedNormClip, TrimmedMean

__all__ = ["setup_strategy", "setup_seed", "base_strategy_lst", "OUT_OF_SCOPE"]

#: names the reference builds with its default trainer (common/utils.py:12), minus the
#: out-of-scope server-side distillation strategies
base_strategy_lst = ["avg", "avgm", "bn", "lg", "lg_r", "opt", "sgd"]
#: registry names of the reference that this engine deliberately does not provide
OUT_OF_SCOPE = ("md", "pav")


def setup_strategy(strategy_name, custom_strategy, **strategy_p):
    """Name -> strategy instance, as common/utils.py:16-58.  Unknown names fall back to
    `custom_strategy`, else SystemError.  Extra keyword arguments understood here:
    shared_key_layers (LG / LG_R), h (Dyn), output / device / devices / group / chunk_clients
    (engine), server_side (AVGM / OPT), trim and server_opt (TrimmedMean; server_opt also Median),
    f, m, center and server_opt (Krum / MultiKrum; f defaults to 0), tau, quantile, center,
    server_opt, noise_multiplier, seed and sequence (NormClip; StreamedNormClip: all but quantile),
    server_opt, delta, stochastic and seed (QuantizedAVG, "avg_q8")."""
    shared_key_layers = strategy_p.get("shared_key_layers", None)
    eng = {k: strategy_p[k] for k in ("output", "device", "devices", "group", "chunk_clients") if k in strategy_p}
    server_side = strategy_p.get("server_side", False)
    h = strategy_p.get("h", None)
    name = strategy_name.lower()
    factories = {
        "avg": lambda: AVG(**eng),
        "avgm": lambda: AVGM(server_side=server_side, **eng),
        "bn": lambda: BN(**eng),
        "distill": lambda: Distill(**eng),
        "dyn": lambda: Dyn(h, **eng),
        "lg": lambda: LG(shared_key_layers, **eng),
        "lg_r": lambda: LG_R(shared_key_layers, **eng),
        "opt": lambda: OPT(server_side=server_side, **eng),
        "sgd": lambda: SGD(**eng),
        "prox": lambda: Prox(**eng),
        "trimmedmean": lambda: TrimmedMean(strategy_p.get("trim", 0.1), strategy_p.get("server_opt"), **eng),
        "median": lambda: Median(strategy_p.get("server_opt"), **eng),
        "krum": lambda: Krum(strategy_p.get("f", 0), strategy_p.get("server_opt"), strategy_p.get("center", "previous"), **eng),
        "multikrum": lambda: MultiKrum(strategy_p.get("f", 0), strategy_p.get("m"), strategy_p.get("server_opt"),
                                       strategy_p.get("center", "previous"), **eng),
        "normclip": lambda: NormClip(strategy_p.get("tau"), strategy_p.get("quantile"), strategy_p.get("server_opt"),
                                     strategy_p.get("center", "previous"), **eng,
                                     noise_multiplier=strategy_p.get("noise_multiplier"), seed=strategy_p.get("seed"),
                                     sequence=strategy_p.get("sequence", 0)),
        "normclip_stream": lambda: StreamedNormClip(
            strategy_p.get("tau"), strategy_p.get("server_opt"), strategy_p.get("center", "previous"),
            **{k: v for k, v in eng.items() if k in ("output", "device")}, chunk_clients=strategy_p.get("chunk_clients", 16),
            noise_multiplier=strategy_p.get("noise_multiplier"), seed=strategy_p.get("seed"),
            sequence=strategy_p.get("sequence", 0)),
        "avg_q8": lambda: QuantizedAVG(
            strategy_p.get("server_opt"), strategy_p.get("delta", True), strategy_p.get("stochastic", False),
            strategy_p.get("seed"), **{k: v for k, v in eng.items() if k in ("output", "device", "chunk_clients")}),
    }
    if name in factories:
        return factories[name]()
    if custom_strategy is not None:
        return custom_strategy
    if name in OUT_OF_SCOPE:
        raise NotImplementedError(
            f"strategy {name!r} trains models on the server and is outside this aggregation engine; "
            "use flearn's implementation"
        )
    raise SystemError("Please input valid strategy name or strategy object!")


def setup_seed(seed):
    """common/utils.py:61-68"""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True
