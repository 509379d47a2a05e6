"""Strategy plugin base — the drop-in surface of flearn/common/strategy/strategy.py:10-210.

Callers (flearn's Server.ensemble, Server.py:140) use exactly the reference's methods:
``client(trainer, agg_weight)``, ``server(ensemble_params_lst, round_)``,
``client_receive(trainer, payload)``, the codec hooks and ``server_exception``.  What changes is
``server_ensemble``: instead of N x K numpy calls on one host core it runs the MI355X aggregation
engine (flearn_amd.aggregator), with results bit-identical to the reference's numpy arithmetic.

Extra keyword arguments (all optional, defaults keep the reference's behaviour):
    output  : "reference" (default) | "float32" | "device"  — see Aggregator
    device  : HIP device for the engine (default: torch's current device)
    devices : several HIP devices: the bucket's columns are split over them, each ingesting and
              reducing its share through its own PCIe link (per-GPU parallel H2D/D2H)
    group   : one process per GPU (torch.distributed initialised, e.g. under torchrun): every
              rank calls server() with the same uploads, packs and reduces only its columns, and
              an RCCL all-gather over xGMI reassembles the global model on every rank
              (flearn_amd.dist; True = the default process group)
    reorder : (attribute, default False) allow the split-N kernel for narrow models with many
              clients — deterministic and within 1e-6 normwise of the reference, not bit-exact
    chunk_clients : K — server() aggregates the round in chunks of K clients (Aggregator.begin_round:
              device memory O(K x model), a round larger than HBM), bit-identical to the default
              (None: one client stack, one launch).  `begin_round(round_)` returns a handle for
              aggregating uploads as they arrive.
"""
from __future__ import annotations

from abc import ABC, abstractmethod

import torch
import torch.distributed as _dist

from .._native import NativeError, NativeUnavailable

#: exceptions that mean "the device or the environment failed", re-raised as they are (they are
#: RuntimeErrors; listed so that the NotImplementedError subclass test below cannot catch them)
_DEVICE_ERRORS = (NativeUnavailable, NativeError, torch.OutOfMemoryError, torch.AcceleratorError,
                  _dist.DistError)
#: what bad client data raises — numpy's errors on the reference's arithmetic (shape/dtype/key
#: mismatches, an empty list), the engine's own validation (bucketplan.py / semantics.py) and the
#: deliberate refusals of unsupported client data (NotImplementedError): these take the
#: reference's server_exception -> SystemExit route (avg.py:28-31).  Everything else — a plain
#: RuntimeError from a gloo/c10d collective (timeout, dead peer), a device-placement error,
#: OSError, ... — is a device or environment failure and propagates unchanged.
_CLIENT_DATA_ERRORS = (ValueError, TypeError, LookupError, AttributeError, ArithmeticError,
                       NotImplementedError, SystemError)


class BaseEncrypt:
    """Identity codec (flearn/common/Encrypt.py:6-13); any object with encode/decode fits."""

    def encode(self, params):
        return params

    def decode(self, glob_params):
        return glob_params


class Strategy(ABC):
    def __init__(self, encrypt=None, output: str = "reference", device=None, devices=None, group=None,
                 chunk_clients=None):
        self.encrypt = BaseEncrypt() if encrypt is None else encrypt
        self.output = output
        self.device = device
        self.devices = devices
        self.group = group
        self.chunk_clients = chunk_clients
        self._engine = None

    # -- engine -----------------------------------------------------------------------------
    @property
    def engine(self):
        """The device Aggregator (created on first use; raises NativeUnavailable without a GPU)."""
        if self.__dict__.get("_engine") is None:
            from ..aggregator import Aggregator

            d = self.__dict__
            self._engine = Aggregator(device=d.get("device"), output=d.get("output", "reference"),
                                      devices=d.get("devices"), group=d.get("group"),
                                      reorder=bool(d.get("reorder", False)), chunk_clients=d.get("chunk_clients"))
        return self._engine

    # -- reference surface ------------------------------------------------------------------
    @staticmethod
    def extract_lst(lst, key):
        return [x[key] for x in lst]

    def server_pre_processing(self, ensemble_params_lst):
        """strategy.py:20-38: split uploads into (agg_weight_lst, w_local_lst), by reference."""
        agg_weight_lst = [p["agg_weight"] for p in ensemble_params_lst]
        w_local_lst = [p["params"] for p in ensemble_params_lst]
        return agg_weight_lst, w_local_lst

    def server_post_processing(self, ensemble_params_lst, ensemble_params, **kwargs):
        return ensemble_params

    def receive_processing(self, data):
        return self.encrypt.decode(data)

    def upload_processing(self, data):
        return self.encrypt.encode(data)

    @staticmethod
    def swa_moving_average(w1, w2, alpha=1.0):
        """strategy.py:80-90 (host helper, not on the aggregation path)."""
        for k in w2.keys():
            w2[k] = w2[k] * alpha + w1[k] * (1 - alpha)
        return w2

    def server_exception(self, e):
        """strategy.py:92-100: report and stop the server (SystemExit)."""
        print(e)
        raise SystemExit("check that the client model parameters are valid")

    def server_ensemble(self, agg_weight_lst, w_local_lst, key_lst=None, server_opt=None):
        """strategy.py:102-130 on the GPU: weighted mean of the uploads over key_lst (default:
        keys common to all clients), in list order, with the reference's numpy dtypes."""
        return self.engine.ensemble(agg_weight_lst, w_local_lst, key_lst, server_opt=server_opt)

    def _ensemble_or_exit(self, ensemble_params_lst, key_lst=None, server_opt=None):
        agg_weight_lst, w_local_lst = self.server_pre_processing(ensemble_params_lst)
        try:
            return self.server_ensemble(agg_weight_lst, w_local_lst, key_lst=key_lst, server_opt=server_opt)
        except _DEVICE_ERRORS:
            # the HIP library or GPU missing, a failed launch, HIP out-of-memory or runtime
            # errors, a failed collective: a device or environment problem, not bad client data —
            # never turned into the "check that the client model parameters are valid" exit
            raise
        except _CLIENT_DATA_ERRORS as e:  # the reference's convention (avg.py:28-31)
            self.server_exception(e)

    # -- a round aggregated as it arrives ------------------------------------------------------
    def _round_spec(self, first_params):
        """(key_lst, server_opt) server() hands the engine for a round whose first upload carries
        `first_params`: the hook begin_round() shares with server()."""
        return None, None

    def _round_done(self, w_glob, uploads):
        """What server() returns for the aggregated w_glob; uploads: the round's upload dicts
        without their "params" (released chunk by chunk)."""
        return {"w_glob": w_glob}

    def begin_round(self, round_):
        """A handle for one round aggregated as uploads arrive: `add(upload)` takes an upload dict
        (or, in HTTP mode, the encoded string: it goes through receive_processing), `finish()` returns
        what `server(all uploads, round_)` returns, bit for bit.  Chunks of `chunk_clients` (16 when
        unset) clients are packed and folded while later uploads are still on their way."""
        return StrategyRound(self, round_)

    @abstractmethod
    def client(self, trainer, agg_weight=1.0):
        return NotImplemented

    @abstractmethod
    def server(self, ensemble_params_lst, round_):
        return NotImplemented

    @abstractmethod
    def client_receive(self, trainer, w_glob_b):
        return NotImplemented


class StrategyRound:
    """Strategy.begin_round's handle (the engine's RoundAccumulator behind the strategy's hooks).
    Client-data errors take server()'s route, server_exception -> SystemExit; device errors propagate.
    server_post_processing sees the uploads without their "params" ({"agg_weight": a, ...} per
    upload): the params are released as soon as their chunk is folded."""

    def __init__(self, strategy, round_):
        self.strategy, self.round_ = strategy, round_
        self._acc = None
        self._seen = []

    def _guard(self, fn, *args):
        try:
            return fn(*args)
        except _DEVICE_ERRORS:
            raise
        except _CLIENT_DATA_ERRORS as e:
            self.strategy.server_exception(e)

    def _begin(self, first_params):
        s = self.strategy
        # (an empty round has no first upload: finish() then raises what server([]) raises)
        key_lst, server_opt = (None, None) if first_params is None else s._round_spec(first_params)
        k = s.__dict__.get("chunk_clients")
        self._acc = s.engine.begin_round(key_lst, server_opt, 16 if k is None else k)

    def add(self, upload):
        if isinstance(upload, (str, bytes, bytearray)):
            upload = self.strategy.receive_processing(upload)
        if self._acc is None:
            self._begin(upload["params"])
        self._guard(self._acc.add, upload)
        self._seen.append({k: v for k, v in upload.items() if k != "params"})

    def finish(self):
        if self._acc is None:
            self._begin(None)
        w_glob = self._guard(self._acc.finish)
        return self.strategy.server_post_processing(self._seen, self.strategy._round_done(w_glob, self._seen))


class ParentStrategy(Strategy):
    """strategy.py:191-210: delegate to a wrapped strategy, sharing its attributes."""

    def __init__(self, strategy):
        self.strategy = strategy
        self.__dict__.update(self.strategy.__dict__)

    def client(self, trainer, agg_weight):
        return self.strategy.client(trainer, agg_weight)

    def server(self, ensemble_params_lst, round_):
        return self.strategy.server(ensemble_params_lst, round_)

    def client_receive(self, trainer, w_glob_b):
        return self.strategy.client_receive(trainer, w_glob_b)

    def begin_round(self, round_):
        return self.strategy.begin_round(round_)
