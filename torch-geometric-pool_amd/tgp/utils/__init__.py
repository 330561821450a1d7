from .ops import (
    add_remaining_self_loops,
    apply_dense_node_mask,
    batched_negative_edge_sampling,
    build_pooled_batch,
    check_and_filter_edge_weights,
    connectivity_to_edge_index,
    connectivity_to_sparsetensor,
    connectivity_to_torch_coo,
    delta_gcn_matrix,
    dense_to_block_diag,
    expand_compacted_rows,
    get_mask_from_dense_s,
    is_dense_adj,
    is_multi_graph_batch,
    negative_edge_sampling,
    postprocess_adj_pool_dense,
    postprocess_adj_pool_sparse,
    pseudo_inverse,
    rank3_diag,
    rank3_trace,
)
from .losses import maxcut_loss
from .signature import Signature, foo_signature

__all__ = [
    "add_remaining_self_loops", "apply_dense_node_mask", "batched_negative_edge_sampling", "build_pooled_batch", "check_and_filter_edge_weights",
    "connectivity_to_edge_index", "connectivity_to_sparsetensor", "connectivity_to_torch_coo",
    "delta_gcn_matrix", "dense_to_block_diag", "expand_compacted_rows", "get_mask_from_dense_s", "is_dense_adj",
    "is_multi_graph_batch", "maxcut_loss", "negative_edge_sampling", "postprocess_adj_pool_dense", "postprocess_adj_pool_sparse", "pseudo_inverse",
    "rank3_diag", "rank3_trace", "Signature", "foo_signature",
]
