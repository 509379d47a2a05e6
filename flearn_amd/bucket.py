"""Every name this module defined before it was split, re-exported as the same object: bucketplan.py
plans the buckets, packer.py copies uploads in and results out, rowtable.py reads device uploads."""
from .bucketplan import (_NP, _PLANS, _PLANS_LOCK, _PLANS_MAX, _STORE, ALIGN, ALIGN_F16, FMT, SMALL_BYTES,  # noqa: F401
                         STRIDE_ALIGN_F16, TORCH_DTYPE, BucketPlan, Group, Piece, Segment, Shard, _as_array_meta,
                         _build_plan, _plain_dicts, _raw_signature, _same_numerics, _same_signature_native, make_plan,
                         rank_width, select_keys, split_columns)
from .packer import AsyncPack, NativeRows, Packer  # noqa: F401
from .rowtable import _ROW_SOURCES, RowTable  # noqa: F401

_NativeRows = NativeRows  # its name before the aggregator imported it at module level
