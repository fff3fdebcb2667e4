"""Covisitation-matrix builder (the component the reference lacks)
behind the reference's script + parquet contract. See ``builder.py`` (CLI),
``engine.py`` (device engine over the C-ABI) and ``parts.py`` (the part files back
into resident matrices, for a consumer process)."""
from .spec import ALL_KINDS, REFERENCE_KINDS, TYPE_WEIGHTS, FILTER_MASKS, Q16  # noqa: F401
