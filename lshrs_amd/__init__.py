"""lshrs_amd — MI355X-native implementation of the lshrs compute hot path.

Drop-in names (same surface as the reference package ``lshrs``):

    LSHRS / lshrs, LSHHasher, HashSignatures, top_k_cosine, cosine_similarity, l2_norm

The arithmetic lives in ``csrc/*.hip`` (gfx950 only; one translation unit per kernel family) behind the C ABI of
``include/lshrs_hip.h``; this package is the Python boundary around it.  There is
no CPU compute path: without the built extension and a visible MI355X every
compute call raises ``lshrs_amd._native.NativeLibraryError``.
"""

from ._config import HashSignatures
from ._exact import exact_above, exact_knn, exact_pairs_above, exact_top_k, scan_epsilon, scan_max_window
from ._groups import exact_groups_above, group_pairs, lsh_groups_above
from ._join import lsh_pairs_above
from ._knn_join import lsh_knn
from ._native import NativeLibraryError
from ._refine import expand_candidates, graph_edges, refine_knn
from .bandrows import get_optimal_config
from .core import LSHRS, lshrs
from .hasher import HostBlasNotRecognised, LSHHasher
from .packed_ops import RedisPackedWriter, group_by_bucket, hex_keys
from .similarity import cosine_similarity, l2_norm, quantize_rows, rerank_batch, top_k_cosine
from .storage import BucketOperation, InMemoryStorage
from .vectors import DeviceVectors

__all__ = [
    "LSHRS", "lshrs", "LSHHasher", "HashSignatures", "top_k_cosine", "cosine_similarity", "l2_norm",
    "rerank_batch", "quantize_rows", "exact_top_k", "exact_above", "exact_pairs_above", "exact_knn", "lsh_pairs_above", "scan_epsilon", "scan_max_window",
    "get_optimal_config", "InMemoryStorage", "BucketOperation", "NativeLibraryError",
    "RedisPackedWriter", "group_by_bucket", "hex_keys", "HostBlasNotRecognised",
    "DeviceVectors", "group_pairs", "exact_groups_above", "lsh_groups_above", "lsh_knn",
    "refine_knn", "graph_edges", "expand_candidates",
]
__version__ = "0.1.0"
