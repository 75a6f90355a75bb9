"""MI355X-native enhanced-suffix-array construction: a drop-in for the hot
path of `gt suffixerator` (GenomeTools).  See DESIGN.md."""
from .esa import EsaEngine, EsaResult, suffixerator_tables  # noqa: F401
from . import synth  # noqa: F401
from .contained import ContainedReads, prefilter  # noqa: F401
from .strgraph import StringGraph, assemble  # noqa: F401
from .kcorrect import KmerCorrection, correct  # noqa: F401
