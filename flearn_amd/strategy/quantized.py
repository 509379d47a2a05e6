"""FedAVG over int8 block-quantized uploads (quant.py, quantround.py)."""
from __future__ import annotations

import numpy as np
import torch

from .. import quant
from .avg import AVG
from .utils import convert_to_np


def _copy_f32(w_glob) -> dict:
    """A copy of a w_glob with every floating value cast to fp32 (the model a client loads): the
    centre delta uploads are taken against, on both sides."""
    out = {}
    for k, v in w_glob.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.detach().to(torch.float32, copy=True) if v.is_floating_point() else v.detach().clone()
        else:
            a = np.asarray(v)
            out[k] = np.array(a, dtype=np.float32) if a.dtype.kind == "f" else np.array(a)
    return out


class QuantizedAVG(AVG):
    """Federated Averaging whose clients upload int8 block-quantized models (FedPAQ, Reisizadeh et
    al. 2020): one byte per fp32 parameter and one fp32 scale per 1024, on the wire, over PCIe and in
    HBM, summed on the device without ever being expanded (Aggregator.ensemble_quantized).  The
    server's result is bit-identical to AVG over the dequantized uploads.

    delta=True: from the second round on a client quantizes its update x - g against the last global
    model it received (cast to fp32), which is what makes 8 bits enough late in training; the server
    keeps its own fp32 copy of the last w_glob as the centre (`init_global(w_glob)` sets the first one,
    for clients that start from a model the server handed out).  Before a client has received a
    w_glob it uploads the quantized model itself.  stochastic=True rounds with QSGD's unbiased rule
    (Alistarh et al. 2017), from numpy.random.default_rng(seed).  server_opt: a ServerOptimizer fused
    into the divide.  A round of plain (unquantized) uploads takes AVG's path unchanged; a round
    mixing the two is refused.  One device; chunk_clients=K folds a quantized round in chunks of K
    clients.  Client-data errors take server_exception's route."""

    def __init__(self, server_opt=None, delta=True, stochastic=False, seed=None, encrypt=None, output="reference",
                 device=None, chunk_clients=None):
        super().__init__(encrypt, output, device, None, None, chunk_clients)
        self.server_opt = server_opt
        self.delta = bool(delta)
        self.stochastic = bool(stochastic)
        self.seed = seed
        self._rng = np.random.default_rng(seed) if stochastic else None
        self._prev_glob = None  # the server's centre: its last w_glob in fp32
        self._received = None  # the client's: the last w_glob it received, in fp32

    def init_global(self, w_glob):
        """The model the first round's delta uploads were taken against (an fp32 copy is kept)."""
        if not hasattr(w_glob, "keys"):
            raise ValueError("init_global takes a w_glob-like dict")
        self._prev_glob = _copy_f32(w_glob)

    def client(self, trainer, agg_weight=1.0):
        """Upload the state_dict quantized: against the last received w_glob when delta is on and
        there is one, else as it is."""
        center = self._received if self.delta else None
        params = quant.quantize_state_dict(convert_to_np(trainer.weight), center, self.stochastic, self._rng)
        return {"agg_weight": agg_weight, "params": params}

    def client_receive(self, trainer, server_p_bytes):
        """AVG's, and an fp32 copy of the received w_glob is kept as the next upload's centre."""
        server_p = super().client_receive(trainer, server_p_bytes)
        self._received = {k: v.numpy() if isinstance(v, torch.Tensor) else v
                          for k, v in _copy_f32({k: v.cpu() if isinstance(v, torch.Tensor) else v
                                                 for k, v in server_p["w_glob"].items()}).items()}
        return server_p

    def server(self, ensemble_params_lst, round_):
        """{"w_glob": the round's mean}; client-data errors -> server_exception, device errors propagate."""
        return {"w_glob": self._ensemble_or_exit(ensemble_params_lst, server_opt=self.server_opt)}

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        if any(quant.is_quantized(w) for w in w_local_lst):
            w_glob = self.engine.ensemble_quantized(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt,
                                                    center=self._prev_glob)
        else:
            w_glob = self.engine.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt)
        self._prev_glob = _copy_f32(w_glob)  # a copy of its own: the caller may change what it is handed
        return w_glob
