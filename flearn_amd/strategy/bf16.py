"""FedAVG over bfloat16 uploads (bf16.py, bf16round.py)."""
from __future__ import annotations

import numpy as np

from .. import bf16
from .avg import AVG


class BF16AVG(AVG):
    """Federated Averaging whose clients upload bfloat16 models (model.bfloat16() trainers, or fp32
    trainers whose uploads are rounded): two bytes per parameter on the wire, over PCIe and in HBM,
    widened in registers and summed in fp32 on the device (Aggregator.ensemble_bf16).  The server's
    result is bit-identical to AVG over the uploads widened to fp32, and it keeps fp32 master weights:
    server_opt, a ServerOptimizer, is fused into the divide.  stochastic=True rounds fp32 weights
    with the unbiased rule, from numpy.random.default_rng(seed); bfloat16 weights are sent as they
    are.  A round of plain uploads takes AVG's path unchanged.  One device; chunk_clients=K folds a
    bfloat16 round in chunks of K clients.  Client-data errors take server_exception's route."""

    def __init__(self, server_opt=None, stochastic=False, seed=None, encrypt=None, output="reference", device=None,
                 chunk_clients=None):
        super().__init__(encrypt, output, device, None, None, chunk_clients)
        self.server_opt = server_opt
        self.stochastic = bool(stochastic)
        self.seed = seed
        self._rng = np.random.default_rng(seed) if stochastic else None

    def client(self, trainer, agg_weight=1.0):
        """Upload the state_dict with every floating tensor as a bfloat16 wire entry."""
        sd = {k: v.detach().cpu() if hasattr(v, "detach") else v for k, v in trainer.weight.items()}
        return {"agg_weight": agg_weight, "params": bf16.encode_state_dict(sd, self.stochastic, self._rng)}

    def server(self, ensemble_params_lst, round_):
        """{"w_glob": the round's mean}; client-data errors -> server_exception, device errors propagate."""
        return {"w_glob": self._ensemble_or_exit(ensemble_params_lst, server_opt=self.server_opt)}

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        return self.engine.ensemble_bf16(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt)
