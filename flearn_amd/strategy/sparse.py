"""FedAVG over top-k sparse uploads (sparse.py, sparseround.py)."""
from __future__ import annotations

import numpy as np
import torch

from .. import sparse
from .avg import AVG
from .quantized import _copy_f32
from .utils import convert_to_np


class TopKAVG(AVG):
    """Federated Averaging whose clients upload the k largest-magnitude coordinates of every fp32 tensor
    (Aji & Heafield 2017; Deep Gradient Compression, Lin et al. 2018): eight bytes per kept entry on the
    wire, over PCIe and in HBM, summed on the device in work proportional to the entries
    (Aggregator.ensemble_sparse).  ratio: the kept fraction per tensor (at least one entry); k: a count
    per tensor instead.

    delta=True: from the second round on a client sparsifies its update x - g against the last global
    model it received (cast to fp32) — the point of the format: an update is compressible, a model is
    not — and the server adds the weighted sparse sum to wsum * g, g being its own fp32 copy of the last
    w_glob (`init_global(w_glob)` sets the first one).  Before a client has received a w_glob it uploads
    the sparsified model itself.  error_feedback (the default; Stich et al. 2018): the client instance
    keeps the fp32 residual e per key, sparsifies x + e (less the centre for delta uploads) and sets e to
    what it sparsified minus what it sent, so nothing it drops is lost.  server_opt: a ServerOptimizer
    fused into the divide.  A round of plain uploads takes AVG's path unchanged; a round mixing formats
    is refused.  One device; chunk_clients=K folds a sparse round in chunks of K clients.  Client-data
    errors take server_exception's route."""

    def __init__(self, server_opt=None, ratio=0.01, k=None, delta=True, error_feedback=True, encrypt=None,
                 output="reference", device=None, chunk_clients=None):
        sparse.top_k_count(1, ratio, k)  # refuses a bad ratio or k
        if error_feedback not in (False, True):
            raise ValueError(f"error_feedback must be True or False, got {error_feedback!r}")
        super().__init__(encrypt, output, device, None, None, chunk_clients)
        self.server_opt = server_opt
        self.ratio = ratio
        self.k = k
        self.delta = bool(delta)
        self.error_feedback = bool(error_feedback)
        self._residual = {}  # the client's: key -> what its last upload sparsified minus what it sent
        self._prev_glob = None  # the server's centre: its last w_glob in fp32
        self._received = None  # the client's: the last w_glob it received, in fp32

    def init_global(self, w_glob):
        """The model the first round's delta uploads were taken against (an fp32 copy is kept)."""
        if not hasattr(w_glob, "keys"):
            raise ValueError("init_global takes a w_glob-like dict")
        self._prev_glob = _copy_f32(w_glob)

    def client(self, trainer, agg_weight=1.0):
        """Upload the state_dict sparsified: against the last received w_glob when delta is on and there
        is one, else as it is."""
        center = self._received if self.delta else None
        sd = convert_to_np(trainer.weight)
        if not self.error_feedback:
            return {"agg_weight": agg_weight, "params": sparse.sparsify_state_dict(sd, center, self.ratio, self.k)}
        fed = {}
        for key, v in sd.items():
            a = np.asarray(v)
            e = self._residual.get(key)
            fed[key] = a + e if a.dtype == np.float32 and e is not None and e.shape == a.shape else v
        params = sparse.sparsify_state_dict(fed, center, self.ratio, self.k)
        for key, entry in params.items():
            if sparse.is_entry(entry):
                u = fed[key] - np.asarray(center[key], dtype=np.float32) if center is not None else np.asarray(fed[key])
                self._residual[key] = u - sparse.densify_entry(dict(entry, delta=False), None, key)
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
        if any(sparse.is_sparse(w) for w in w_local_lst):
            w_glob = self.engine.ensemble_sparse(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt,
                                                 center=self._prev_glob)
        else:
            w_glob = self.engine.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt)
        self._prev_glob = _copy_f32(w_glob)  # a copy of its own: the caller may change what it is handed
        return w_glob
