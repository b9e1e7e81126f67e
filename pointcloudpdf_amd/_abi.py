"""The parameter lists of the C ABI that include/pdfops.h declares, as one table (data only: nothing but ctypes is imported).

``ENTRIES`` maps every declared symbol to ``(ret, kinds)``.  ``kinds`` is the header's complete parameter list, the trailing
``void *stream`` included: "i" int / unsigned, "l" long, "f" float, "d" double, "p" any pointer.  ``ret``: "s" an int status
(0 = PDF_OK, negative = PDF_ERR_*), "i" an int value, "l" a long value, "z" a ``const char *``.  A wrong row hands shifted arguments
to a kernel, so tests/test_abi.py parses the header and holds this table equal to it, row for row; nothing reads the header at run time.
"""
import ctypes

_KIND = {"i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "d": ctypes.c_double, "p": ctypes.c_void_p}
_RET = {"s": ctypes.c_int, "i": ctypes.c_int, "l": ctypes.c_long, "z": ctypes.c_char_p}

ENTRIES = {
    # csrc/api.hip
    "pdf_abi_version": ("i", ""),
    "pdf_build_info": ("z", ""),
    # csrc/knn_query.hip
    "pdf_dist_fma_mode": ("i", ""),
    "pdf_knn_query": ("s", "iippppippp"),
    "pdf_knn_query_list": ("s", "iippppippppp"),
    # csrc/knn_grid.hip
    "pdf_knn_workspace_bytes": ("l", "iii"),
    "pdf_knn_grid_supported": ("i", "i"),
    "pdf_knn_query_ws": ("s", "iiippppippplp"),
    "pdf_knn_grid_build": ("s", "ippiplp"),
    "pdf_knn_query_grid": ("s", "iiippppippplp"),
    "pdf_knn_query_ws_counted": ("s", "iiippppippplpp"),
    "pdf_radius_neighbors_self": ("s", "iifppippplp"),
    "pdf_radius_neighbors_self_adaptive": ("s", "iiffppipppplp"),
    # csrc/ball_query.hip
    "pdf_ball_query": ("s", "iiffppppippp"),
    "pdf_random_ball_query": ("s", "iiffpppppippp"),
    # csrc/sampling.hip
    "pdf_farthest_point_sampling": ("s", "ii" + "p" * 6),
    "pdf_fps_reference_block_log2": ("i", "i"),
    # csrc/sampling_bucketed.hip
    "pdf_fps_workspace_bytes": ("l", "ii"),
    "pdf_fps_stats_offset": ("l", "ii"),
    "pdf_farthest_point_sampling_bucketed": ("s", "iiipppplpp"),
    # csrc/gather_ops.hip
    "pdf_grouping_forward": ("s", "iiipppp"),
    "pdf_grouping_backward": ("s", "iiipppp"),
    "pdf_grouping_forward_ordered": ("s", "iiippppp"),
    "pdf_group_forward_ordered": ("s", "iiii" + "p" * 7),
    "pdf_interpolation_forward_ordered": ("s", "iii" + "p" * 6),
    "pdf_subtraction_forward_ordered": ("s", "iii" + "p" * 6),
    "pdf_aggregation_forward_ordered": ("s", "iiii" + "p" * 7),
    "pdf_interpolation_forward": ("s", "iiippppp"),
    "pdf_interpolation_backward": ("s", "iiippppp"),
    "pdf_subtraction_forward": ("s", "iiippppp"),
    "pdf_subtraction_backward": ("s", "iiippppp"),
    "pdf_aggregation_forward": ("s", "iiii" + "p" * 6),
    "pdf_aggregation_backward": ("s", "iiii" + "p" * 9),
    "pdf_group_forward": ("s", "iiii" + "p" * 6),
    "pdf_group_backward": ("s", "iiiipppp"),
    "pdf_interpolation_weights": ("s", "iippp"),
    # csrc/attention.hip
    "pdf_attention_relation_step_forward": ("s", "iii" + "p" * 7),
    "pdf_attention_relation_step_backward": ("s", "iii" + "p" * 10),
    "pdf_attention_fusion_step_forward": ("s", "iii" + "p" * 6),
    "pdf_attention_fusion_step_backward": ("s", "iii" + "p" * 8),
    # csrc/fused_layer.hip
    "pdf_pt_layer_supported": ("i", "ii"),
    "pdf_pt_layer_partial_floats": ("l", "iii"),
    "pdf_pt_layer_forward": ("s", "iii" + "p" * 8 + "iffpppppipp"),
    "pdf_pt_layer_forward_m": ("s", "iii" + "p" * 8 + "iffpppppipppp"),
    "pdf_pt_layer_bwd_partial_floats": ("l", "iii"),
    "pdf_pt_layer_bwd_sums_floats": ("l", "i"),
    "pdf_pt_layer_backward": ("s", "iii" + "p" * 19 + "ippippp"),
    # csrc/pointwise.hip
    "pdf_bn_supported": ("i", "i"),
    "pdf_bn_act_forward": ("s", "li" + "p" * 6 + "iffipppp"),
    "pdf_bn_act_backward": ("s", "lippppiippppp"),
    "pdf_bn_coef": ("s", "lipppppiffppp"),
    "pdf_bn_apply": ("s", "lipppipp"),
    "pdf_bn_coef_from_partial": ("s", "pilippppffpp"),
    "pdf_bn_act_backward_presummed": ("s", "lipppiipippp"),
    "pdf_bn_coef_from_partial2": ("s", "iliilipffp"),
    "pdf_bn_act_backward2": ("s", "lilipip"),
    "pdf_bn_bwd_sums": ("s", "lipppippp"),
    # csrc/block.hip
    "pdf_bn_partial_floats": ("l", "li"),
    "pdf_rowlin_partial_floats": ("l", "li"),
    "pdf_rowlin_wgrad_ws_floats": ("l", "liii"),
    "pdf_bn_coef_eval_or_partial": ("s", "pilippppiffpp"),
    "pdf_block_pre_forward": ("s", "lipiffip"),
    "pdf_block_pre_backward": ("s", "lipiip"),
    "pdf_block_post_forward": ("s", "lipiffip"),
    "pdf_block_post_backward": ("s", "lipiip"),
    "pdf_bottleneck_forward": ("s", "liipiffiip"),
    "pdf_bottleneck_backward": ("s", "liipiiiip"),
    "pdf_linbn_forward": ("s", "liipiiffip"),
    "pdf_linbn_backward": ("s", "liipiiip"),
    "pdf_transition_up_supported": ("i", "iii"),
    "pdf_transition_up_forward": ("s", "liliipiffip"),
    "pdf_transition_up_backward": ("s", "liliipiip"),
    # csrc/rowlin.hip
    "pdf_rowlin_partial_rows": ("i", "lii"),
    "pdf_rowlin_forward": ("s", "liiplpipppiplipip"),
    "pdf_rowlin_wgrad": ("s", "liiplplppipppip"),
    "pdf_rowlin_multi": ("s", "liiiiplpipppipliip"),
    "pdf_rowlin_wgrad_multi": ("s", "liiiplplppipppip"),
    "pdf_rowlin_wgrad_group": ("s", "liiiplpl" + "p" * 6 + "ip"),
    "pdf_rowlin_wgrad_group_dgrad": ("s", "liiiplpl" + "p" * 6 + "pppipip"),
    "pdf_rowlin_dgrad_bstats": ("s", "liiiplpplplpippip"),
    "pdf_rowlin_forward_bn": ("s", "liiplppppiplpppppffpip"),
    "pdf_rowlin_wgrad2": ("s", "liiliipip"),
    "pdf_rowlin_forward_stats2": ("s", "liliippip"),
    "pdf_rowlin_dgrad2": ("s", "liliippip"),
    "pdf_rowlin_wgrad2_paired": ("s", "liiliippip"),
    "pdf_rowlin_wgrad2_roww": ("s", "liiliipplpip"),
    "pdf_rowlin_forward_roww": ("s", "liiplpipliplip"),
    "pdf_rowlin_wgrad_roww": ("s", "liiplplpplpip"),
    # csrc/kpconv.hip
    "pdf_kpconv_supported": ("i", "ii"),
    "pdf_kpconv_gather": ("s", "iiiipppppfpp"),
    "pdf_kpconv_scatter": ("s", "iiiipppppfpp"),
    # csrc/transition_down.hip
    "pdf_td_supported": ("i", "iii"),
    "pdf_td_tables": ("s", "li" + "p" * 7 + "lppip"),
    "pdf_td_gram_floats": ("l", "i"),
    "pdf_td_fwd_scratch_floats": ("l", "li"),
    "pdf_td_bwd_scratch_floats": ("l", "lii"),
    "pdf_td_forward": ("s", "lliipiffip"),
    "pdf_td_backward": ("s", "lliipiip"),
    # csrc/seg_gather.hip
    "pdf_seg_sum_rows": ("s", "lipppifpp"),
    "pdf_seg_sum_rows_own": ("s", "liipppifpppp"),
    "pdf_seg_sum_rows_strided": ("s", "liplppifpp"),
    "pdf_seg_sum_rows_x": ("s", "liplippifpp"),
    "pdf_seg_sum_weighted_x": ("s", "liiippippippp"),
    "pdf_seg_sum_weighted_ordered": ("s", "liiippppippp"),
    "pdf_seg_sum_weighted": ("s", "liiippppipp"),
    # csrc/loss.hip
    "pdf_ce_workspace_floats": ("l", ""),
    "pdf_ce_forward": ("s", "lipplpppp"),
    "pdf_ce_backward": ("s", "lippppp"),
    "pdf_vote_accumulate": ("s", "li" + "p" * 7),
    # csrc/criteria.hip
    "pdf_criteria_workspace_floats": ("l", "i"),
    "pdf_ce_ex_forward": ("s", "lipppfilpppp"),
    "pdf_ce_ex_backward": ("s", "lipppipp"),
    "pdf_focal_forward": ("s", "lipppffilpppp"),
    "pdf_focal_backward": ("s", "lippppp"),
    "pdf_dice_forward": ("s", "lippfflpppp"),
    "pdf_dice_backward": ("s", "lipplfpppp"),
    "pdf_bfocal_forward": ("s", "lppffiipppp"),
    "pdf_bfocal_backward": ("s", "lpppipp"),
    # csrc/cac.hip
    "pdf_cac_supported": ("i", "ii"),
    "pdf_cac_workspace_floats": ("l", "liii"),
    "pdf_cac_soft_proto_forward": ("s", "liiipppfpppp"),
    "pdf_cac_soft_proto_backward": ("s", "liiipppf" + "p" * 6),
    "pdf_cac_label_proto_forward": ("s", "lii" + "p" * 7),
    "pdf_cac_label_proto_backward": ("s", "liippppp"),
    "pdf_cac_cosine_forward": ("s", "liiipppfpp"),
    "pdf_cac_cosine_backward": ("s", "liiipppfppppp"),
    "pdf_cac_distill_workspace_floats": ("l", "i"),
    "pdf_cac_distill_forward": ("s", "lipppfppppp"),
    "pdf_cac_distill_backward": ("s", "li" + "p" * 6),
    # csrc/sparse_conv.hip
    "pdf_spconv_geometry_workspace_bytes": ("l", "l"),
    "pdf_spconv_bucket_rows": ("l", "l"),
    "pdf_spconv_sort_sites": ("s", "l" + "p" * 6),
    "pdf_spconv_subm_table": ("s", "lppppipp"),
    "pdf_spconv_down": ("s", "l" + "p" * 14),
    "pdf_spconv_supported": ("i", "iii"),
    "pdf_spconv_gather": ("s", "llliiippippplllppp"),
    "pdf_spconv_small_forward": ("s", "liii" + "p" * 6),
    "pdf_spconv_small_dgrad": ("s", "liiippppp"),
    "pdf_spconv_wgrad_ws_floats": ("l", "liii"),
    "pdf_spconv_wgrad": ("s", "lliiipppippp"),
    "pdf_spconv_colsum_ws_floats": ("l", "i"),
    "pdf_spconv_colsum": ("s", "lipppp"),
    # csrc/incr_distill.hip
    "pdf_incr_kl_workspace_floats": ("l", ""),
    "pdf_incr_kl_forward": ("s", "liippplffpppp"),
    "pdf_incr_kl_backward": ("s", "lippppp"),
    # csrc/lovasz.hip
    "pdf_lovasz_workspace_bytes": ("l", "li"),
    "pdf_lovasz_forward": ("s", "lippl" + "p" * 6),
    "pdf_lovasz_backward": ("s", "lippfpp"),
    # csrc/openset_metrics.hip
    "pdf_openset_metrics_workspace_bytes": ("l", "li"),
    "pdf_openset_metrics": ("s", "lipppplpipppp"),
    # csrc/geom_moments.hip
    "pdf_knn_rel_moments_ws_doubles": ("l", "il"),
    "pdf_knn_rel_moments": ("s", "ili" + "p" * 6),
    "pdf_knn_rel_moments_q": ("s", "ili" + "p" * 7),
    "pdf_scene_morton_keys": ("s", "lippppp"),
    # csrc/optim.hip
    "pdf_sgd_chunk": ("i", ""),
    "pdf_sgd_step": ("s", "ippfffpp"),
    "pdf_grad_unscale": ("s", "ippppp"),
    "pdf_scaler_update": ("s", "ppppffip"),
    "pdf_adam_step": ("s", "iippdddddipp"),
    "pdf_adam_grad_unscale": ("s", "ippppp"),
    # csrc/window_attention.hip (the libs/pointops2 launchers declare `unsigned n_max`: same width, bound as "i")
    "pdf_attention_step1_forward_v2": ("s", "iiiii" + "p" * 6),
    "pdf_attention_step1_backward_v2": ("s", "iiiii" + "p" * 8),
    "pdf_dot_prod_with_idx_forward_v3": ("s", "iiiii" + "p" * 9),
    "pdf_dot_prod_with_idx_backward_v3": ("s", "iiiii" + "p" * 13),
    "pdf_attention_step2_with_rel_pos_value_forward_v2": ("s", "iiiii" + "p" * 8),
    "pdf_attention_step2_with_rel_pos_value_backward_v2": ("s", "iiiii" + "p" * 11),
    "pdf_dot_prod_with_idx_forward_v3_l": ("s", "iiiii" + "p" * 9),
    "pdf_dot_prod_with_idx_backward_v3_l": ("s", "iiiii" + "p" * 13),
    "pdf_attention_step2_with_rel_pos_value_backward_v2_l": ("s", "iiiii" + "p" * 11),
    "pdf_segment_softmax_forward": ("s", "iiipppp"),
    "pdf_segment_softmax_backward": ("s", "iiippppp"),
    # csrc/voxel_hash.hip
    "pdf_grid_hash": ("s", "lippdddipppp"),
    # csrc/augment.hip
    "pdf_grid_hash_f64": ("s", "lippdddpppp"),
    "pdf_philox4x64": ("s", "llllpp"),
    "pdf_aug_bounds_workspace_doubles": ("i", "i"),
    "pdf_aug_bounds": ("s", "i" + "p" * 6),
    "pdf_aug_points": ("s", "ilpi" + "p" * 7),
    "pdf_aug_keys": ("s", "ilpplpp"),
    "pdf_aug_elastic_noise": ("s", "ilpplpp"),
    "pdf_aug_elastic_blur": ("s", "ilpppip"),
    "pdf_aug_elastic_apply": ("s", "ilpppppdppp"),
    # csrc/fragments.hip
    "pdf_fragment_bounds_ws_doubles": ("l", "i"),
    "pdf_fragment_bounds": ("s", "lliii" + "p" * 7),
    "pdf_fragment_gather": ("s", "lliiipppppi" + "p" * 9),
    "pdf_fragment_vote": ("s", "lliii" + "p" * 10),
    # csrc/graph_prune.hip
    "pdf_graph_forest_workspace_bytes": ("l", "lll"),
    "pdf_graph_forest": ("s", "lipppppippplp"),
    "pdf_gmm2_1d": ("s", "ipppiddp"),
    "pdf_graph_forest_dev": ("s", "lipppppipppplp"),
    "pdf_gmm2_1d_dev": ("s", "ippppiddp"),
    "pdf_graph_forest_batch_dev": ("s", "ippi" + "p" * 6 + "ippplp"),
    "pdf_gmm2_weak_dev": ("s", "i" + "p" * 8 + "iddp"),
    # csrc/window_attention_bwd.hip
    "pdf_wa_segment_rows": ("s", "iiii" + "p" * 6 + "lfpplfp"),
    "pdf_wa_segment_rows_ordered": ("s", "iiii" + "p" * 6 + "lfpplfpp"),
    "pdf_wa_table_grad_ws_floats": ("l", "iii"),
    "pdf_wa_table_grad": ("s", "iiiippppplfppp"),
    "pdf_wa_grad_attn": ("s", "iiiiiplppplpppp"),
    "pdf_wa_logits_forward": ("s", "iiiiipplf" + "p" * 7),
    "pdf_wa_permute_edges": ("s", "iipppp"),
    "pdf_wa_logits_forward_ordered": ("s", "iiiiipplf" + "p" * 8),
    "pdf_wa_grad_attn_ordered": ("s", "iiiiiplppplppppp"),
    # csrc/window_edges.hip
    "pdf_window_keys": ("s", "ippippfipppp"),
    "pdf_scene_bounds": ("s", "ippippp"),
    "pdf_window_keys_scene": ("s", "ippippfipppp"),
    "pdf_window_edges_count": ("s", "ippi" + "p" * 7),
    "pdf_window_edges_fill": ("s", "i" + "p" * 7 + "ffippppp"),
    # csrc/region_grow.hip
    "pdf_region_stats": ("s", "ippppifpppp"),
    "pdf_region_seeds": ("s", "ippppipp"),
    "pdf_region_grow": ("s", "ippipppipiippppp"),
    "pdf_region_edges": ("s", "ipppppi" + "p" * 12 + "lp"),
    "pdf_region_grow_list_points": ("l", ""),
    "pdf_region_tree": ("s", "ippi" + "p" * 10),
    "pdf_sort_floats_dev": ("s", "i" + "p" * 7),
    "pdf_region_mask": ("s", "i" + "p" * 8),
    # csrc/scene_rows.hip
    "pdf_scene_sum_rows": ("s", "ipiplipp"),
    "pdf_scene_repeat_rows": ("s", "iplipipp"),
    # csrc/layernorm.hip
    "pdf_layernorm_supported": ("i", "i"),
    "pdf_layernorm_partial_floats": ("l", "li"),
    "pdf_layernorm_forward": ("s", "lipppfpppp"),
    "pdf_layernorm_backward": ("s", "li" + "p" * 10),
    # csrc/stage_copy.hip: (count, PdfCopySeg *segments, stream)
    "pdf_stage_copy": ("s", "ipp"),
    # csrc/grid_pool.hip
    "pdf_grid_pool_workspace_bytes": ("l", "l"),
    "pdf_grid_pool_partition": ("s", "lppippf" + "p" * 6),
    "pdf_grid_pool_reduce": ("s", "lli" + "p" * 8),
    "pdf_grid_pool_max_backward": ("s", "llippppp"),
    "pdf_grid_unpool_forward": ("s", "llipppp"),
    # csrc/gva.hip
    "pdf_gva_supported": ("i", "iii"),
    "pdf_gva_relation_forward": ("s", "llii" + "p" * 7),
    "pdf_gva_relation_backward": ("s", "llii" + "p" * 11),
    "pdf_gva_attend_forward": ("s", "lliii" + "p" * 7),
    "pdf_gva_attend_backward": ("s", "lliii" + "p" * 11),
    # csrc/serial_attention.hip
    "pdf_serial_attn_supported": ("i", "iii"),
    "pdf_serial_attn_forward": ("s", "liifpppippp"),
    "pdf_serial_attn_backward": ("s", "liif" + "p" * 6 + "ipippp"),
    # csrc/serialization.hip
    "pdf_serial_workspace_bytes": ("l", "l"),
    "pdf_serial_codes": ("s", "liiipppp"),
    "pdf_serial_sort": ("s", "lippppp"),
    "pdf_serial_pool_partition": ("s", "li" + "p" * 9),
    # csrc/point_group.hip
    "pdf_pg_ball_workspace_bytes": ("l", "ii"),
    "pdf_pg_ball_count": ("s", "iifppppplp"),
    "pdf_pg_ball_fill": ("s", "iifppplpplp"),
    "pdf_pg_cluster_labels": ("s", "ipplpi" + "p" * 8),
    "pdf_pg_cluster_fill": ("s", "llpppp"),
    "pdf_pg_proposals_select": ("s", "ipipppp"),
    "pdf_pg_proposals_fill": ("s", "ililpppppl" + "p" * 8),
    "pdf_pg_intersections": ("s", "llii" + "p" * 8),
    "pdf_pg_bias_loss_workspace_doubles": ("l", ""),
    "pdf_pg_bias_loss_forward": ("s", "lpppiplppppp"),
    "pdf_pg_bias_loss_backward": ("s", "lppppipp"),
    # csrc/scene_contrast.hip
    "pdf_msc_nce_supported": ("i", "i"),
    "pdf_msc_nce_saved_floats": ("l", "li"),
    "pdf_msc_nce_workspace_bytes": ("l", "lii"),
    "pdf_msc_nce_forward": ("s", "lillpppfppplp"),
    "pdf_msc_nce_backward": ("s", "lillpppfppppplp"),
    "pdf_msc_recon_supported": ("i", "i"),
    "pdf_msc_recon_acc_doubles": ("l", ""),
    "pdf_msc_recon_slab_floats": ("l", "li"),
    "pdf_msc_recon_forward": ("s", "llii" + "p" * 12),
    "pdf_msc_recon_backward": ("s", "lli" + "p" * 14),
}


class PdfCopySeg(ctypes.Structure):   # include/pdfops.h: PdfCopySeg, the element of pdf_stage_copy's segment array
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("nbytes", ctypes.c_long), ("src_offset", ctypes.c_void_p),
                ("sub", ctypes.c_void_p), ("sub_const", ctypes.c_int), ("src_elems", ctypes.c_int)]


# the launchers of libs/pointops and libs/pointops2 that the CPU oracle (oracle/pdfops_oracle.c) implements as well
REFERENCE_OPS = (
    "knn_query", "ball_query", "random_ball_query", "farthest_point_sampling",
    "grouping_forward", "grouping_backward", "interpolation_forward", "interpolation_backward",
    "subtraction_forward", "subtraction_backward", "aggregation_forward", "aggregation_backward",
    "attention_relation_step_forward", "attention_relation_step_backward",
    "attention_fusion_step_forward", "attention_fusion_step_backward",
    "attention_step1_forward_v2", "attention_step1_backward_v2", "dot_prod_with_idx_forward_v3", "dot_prod_with_idx_backward_v3",
    "attention_step2_with_rel_pos_value_forward_v2", "attention_step2_with_rel_pos_value_backward_v2",
    "segment_softmax_forward", "segment_softmax_backward",
)


def bind(lib, names=None, prefix="pdf_", stream=True, overrides=None):
    """Set ``restype`` / ``argtypes`` of ``lib``'s functions from the table: every entry, or the short ``names`` (without "pdf_") of a
    library that exports them under ``prefix``.  ``stream=False``: a library without the trailing stream argument; ``overrides``:
    short name -> the kinds of a launcher whose parameter list differs there.  -> {short name: function} of the status entries."""
    overrides = overrides or {}
    status = {}
    for short in (n[4:] for n in ENTRIES) if names is None else names:
        ret, kinds = ENTRIES["pdf_" + short]
        kinds = overrides.get(short, kinds if stream else kinds[:-1])
        fn = getattr(lib, prefix + short)
        fn.restype = _RET[ret]
        fn.argtypes = [_KIND[k] for k in kinds]
        if ret == "s":
            status[short] = fn
    return status
