"""Context: one handle, every family's commands."""

from __future__ import annotations

from .core import _ContextCore
from .genes import _GenesCalls
from .merge import _MergeCalls
from .pileup import _PileupCalls
from .reads import _ReadsCalls
from .sites import _SitesCalls
from .species import _SpeciesCalls


class Context(_SitesCalls, _GenesCalls, _SpeciesCalls, _MergeCalls, _PileupCalls, _ReadsCalls, _ContextCore):
    """One GPU.  Replaces a `mp.Pool` worker and its module globals (midas/run/snps.py:142,167-176)."""
