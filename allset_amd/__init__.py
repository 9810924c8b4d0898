"""allset_amd -- MI355X-native implementation of AllSet's vertex<->hyperedge multiset aggregation
(HalfNLHconv / PMA) behind the reference's own module surface.  HIP kernels live in ``csrc/`` behind
the C ABI of ``include/allset_hip.h``; there is no CPU or eager fallback on the aggregation path."""
from .incidence import Incidence, LeaveOneOutIncidence, cached_incidence          # noqa: F401
from .functional import clique_propagate, deepsets_aggregate, deepsets_aggregate_exclude_self, gat_propagate, hattn_propagate, pma_aggregate, pma_aggregate_exclude_self, pma_attention_weights, scaled_propagate, unigcn_hop   # noqa: F401
from .layers import MLP, PMA, HalfNLHconv, glorot, zeros    # noqa: F401
from .models import SetGNN                                  # noqa: F401
from .baselines import (CEGAT, CEGCN, GATConv, GCNConv, HCHA, HNHN, HNHNConv, HypergraphAttentionConv, HypergraphConv, ImplicitCEGraph,  # noqa: F401
                        UniGCNII, UniGCNIIConv)

__version__ = "0.1.0"
