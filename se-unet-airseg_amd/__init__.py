"""se-unet-airseg_amd: MI355X-native (gfx950) SE-UNet training / inference hot path.

Drop-in for the reference's ``SE_UNet.py`` module surface and ``train.py`` loss functions, backed by
hand-written HIP kernels behind a C ABI (``include/seunet_hip.h``).  The directory name is not a valid
Python identifier; import it as ``seunet_amd`` (alias module at the repo root) or via
``importlib.import_module("se-unet-airseg_amd")``.
"""
from . import _lib, components, ddp, mesh, morphometry, online, ops, optim, pipeline, postprocess, prep, preprocess, topology
from .SE_UNet import CapturedForward, CATConv, DropLayer, SE_UNet, SSEConv, SSEConv2, get_model, load_reference_checkpoint
from .optim import AdamW
from .pipeline import (AirwayHMData3GPU, AirwayHMDataGPU, CropSegDataGPU, aug_code, crop_batch, draw_stage1_plan, draw_stage2_plan,
                       draw_stage3_plan, two_channel_volume)
from .prep import (CandidateSet, airway_parse, binary_closing, binary_dilation, binary_erosion, binary_fill_holes, break_weight,
                   distance_transform_edt, hard_mining_candidates, label_adjacency, lib_weight, relabel, skeleton_parsing, skeletonize_3d,
                   tree_parsing, tree_parsing_func)
from .mesh import (LabelMeshes, branch_meshes, label_meshes, marching_cubes, mesh_adjacency, prediction_mesh, smooth_mesh, stl_records,
                   transform_mesh, write_stl)
from .morphometry import (AirwayWalls, BranchTable, CrossSections, airway_walls, branch_morphometry, branch_stats, branch_tree,
                          branch_wall_distance, cross_sections)
from .preprocess import cut_mask, get_l, large_connected_domain26, preprocess_ct, th_2t
from .postprocess import (MetricSums, SurfaceMetrics, cldice_score, double_threshold_iteration, evaluation_case, largest_component,
                          maximum_3d, order_statistics, postprocess_prediction, surface_distances, surface_metrics, zero_borders)
from .components import (BettiError, ComponentTable, betti_error, betti_numbers, euler_number, label, remove_small_objects)
from .losses import atr_loss, dice_loss, fused_logit_loss, fused_stage_loss, general_union_loss_lib, per_sample_loss, soft_cldice_loss, soft_skeleton
from .online import OnlineHardPool
from .sliding_window import sliding_window_predict, sliding_window_validate, two_channel, window_starts, window_table

__all__ = ["SE_UNet", "SSEConv", "SSEConv2", "CATConv", "DropLayer", "get_model", "load_reference_checkpoint", "dice_loss",
           "general_union_loss_lib", "atr_loss", "fused_logit_loss", "fused_stage_loss", "per_sample_loss", "OnlineHardPool",
           "sliding_window_predict", "sliding_window_validate", "two_channel", "window_starts", "window_table", "AdamW", "CropSegDataGPU", "AirwayHMDataGPU", "AirwayHMData3GPU", "aug_code", "crop_batch", "draw_stage1_plan", "draw_stage2_plan", "draw_stage3_plan", "two_channel_volume", "double_threshold_iteration", "postprocess_prediction", "zero_borders", "maximum_3d", "largest_component",
           "evaluation_case", "MetricSums", "CandidateSet", "distance_transform_edt", "hard_mining_candidates", "lib_weight",
           "break_weight", "skeletonize_3d", "skeleton_parsing", "tree_parsing_func", "label_adjacency", "tree_parsing", "relabel", "airway_parse", "binary_dilation",
           "binary_erosion", "binary_closing", "binary_fill_holes", "preprocess_ct", "th_2t", "get_l", "large_connected_domain26", "cut_mask",
           "marching_cubes", "smooth_mesh", "write_stl", "prediction_mesh", "mesh_adjacency", "stl_records", "transform_mesh",
           "label_meshes", "branch_meshes", "LabelMeshes", "branch_stats", "branch_tree", "branch_morphometry", "BranchTable", "branch_wall_distance",
           "cross_sections", "CrossSections", "airway_walls", "AirwayWalls",
           "soft_skeleton", "soft_cldice_loss", "cldice_score", "surface_distances", "order_statistics", "surface_metrics", "SurfaceMetrics",
           "label", "remove_small_objects", "euler_number", "betti_numbers", "betti_error", "ComponentTable", "BettiError"]
