"""ctypes binding of libinvr.so (include/invr.h).  PyTorch-ROCm tensors in, tensors out.

The library is the product path: if it is missing this module raises at import (no CPU
fallback).  ``lib()`` loads it lazily so that CPU-only host logic (config, params, scene,
state_dict handling) stays importable on a box without the .so or without a GPU.
"""
import ctypes as C
import os

import torch

from . import params
from .config import NUM_PARTS, PART_NAMES

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('INVR_LIB_PATH') or os.path.join(HERE, 'libinvr.so')      # (INVR_LIB_PATH: experiment builds)

MAX_LEVELS, MAX_LINEAR, STATS_LEN = 16, 4, 16
DF_SLICE_MAX = 4096      # csrc/pipeline.h: float2 entries of the deformer's per-frame slice table (InvrWsLayout.dslice)
_f32p, _f64p, _i32p, _i64p, _u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)


class InvrGrid(C.Structure):
    _fields_ = [('dense', C.c_void_p), ('hash', C.c_void_p), ('bounds', C.c_void_p),
                ('n_levels', C.c_int32), ('n_features', C.c_int32), ('start_hash', C.c_int32),
                ('separate_dense', C.c_int32), ('table_len', C.c_int64),
                ('res', C.c_int32 * MAX_LEVELS), ('cell', C.c_float * MAX_LEVELS),
                ('dense_off', C.c_int64 * MAX_LEVELS),
                ('sum', C.c_int32), ('sum_over_features', C.c_int32), ('include_input', C.c_int32),
                ('vertex_rows', C.c_int32), ('row_sums', C.c_void_p)]


class InvrMlpBwdOut(C.Structure):
    _fields_ = [('g_emb', C.c_void_p), ('gz', C.c_void_p), ('a', C.c_void_p), ('n_pad', C.c_int64), ('g_latent', C.c_void_p)]


class InvrDeformBwdOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('uvt', 'gfeat', 'gz1', 'gz2', 'gz3', 'a0', 'a1', 'a2')]


class InvrAdamTensor(C.Structure):
    _fields_ = [('param', C.c_void_p), ('grad', C.c_void_p), ('exp_avg', C.c_void_p), ('exp_avg_sq', C.c_void_p),
                ('numel', C.c_int64), ('lr', C.c_float), ('weight_decay', C.c_float), ('bc1', C.c_float), ('bc2_sqrt', C.c_float),
                ('active', C.c_void_p), ('grad_shift', C.c_int32), ('step', C.c_int32)]


class InvrPartGrads(C.Structure):
    _fields_ = [('row_grad', C.c_void_p), ('occ_w', C.c_void_p * 4), ('occ_b', C.c_void_p * 4), ('rgb_w', C.c_void_p * 4),
                ('rgb_b', C.c_void_p * 4), ('rgb_latent', C.c_void_p)]


class InvrTrainGrads(C.Structure):
    _fields_ = [('part', InvrPartGrads * NUM_PARTS), ('deform_dense', C.c_void_p), ('deform_hash', C.c_void_p),
                ('deform_w', C.c_void_p * 4), ('deform_b', C.c_void_p * 4), ('part_active', C.c_void_p)]


class InvrMlp(C.Structure):
    _fields_ = [('weight', C.c_void_p * MAX_LINEAR), ('bias', C.c_void_p * MAX_LINEAR),
                ('dims', C.c_int32 * (MAX_LINEAR + 1)), ('n_linear', C.c_int32)]


class InvrPart(C.Structure):
    _fields_ = [('grid', InvrGrid), ('occ', InvrMlp), ('rgb', InvrMlp), ('rgb_latent', C.c_void_p),
                ('latent_dim', C.c_int32), ('num_latent_code', C.c_int32)]


class InvrModel(C.Structure):
    _fields_ = [('part', InvrPart * NUM_PARTS), ('deform_grid', InvrGrid), ('deform_mlp', InvrMlp),
                ('n_dir_freq', C.c_int32), ('geo_feature_dim', C.c_int32)]


class InvrScene(C.Structure):
    _fields_ = [('R', C.c_void_p), ('Th', C.c_void_p), ('A', C.c_void_p), ('big_A', C.c_void_p),
                ('pbw', C.c_void_p), ('pbw_dims', C.c_int32 * 3), ('pbw_channels', C.c_int32),
                ('pbounds', C.c_void_p), ('tuv', C.c_void_p), ('tuv_dims', C.c_int32 * 3),
                ('tbounds', C.c_void_p), ('part_pts', C.c_void_p), ('part_pbw', C.c_void_p),
                ('lengths2', C.c_void_p), ('part_stride', C.c_int32), ('frame_dim', C.c_void_p),
                ('latent_index', C.c_void_p), ('smpl_thresh', C.c_float), ('tpose_viewdir', C.c_int32),
                ('composite_eps', C.c_float), ('aggr', C.c_int32)]


class InvrWsLayout(C.Structure):
    _fields_ = [('cap', C.c_int64), ('lcap', C.c_int64), ('counters', C.c_int64), ('active_idx', C.c_int64),
                ('word_off', C.c_int64), ('mask', C.c_int64), ('pflags', C.c_int64), ('farflags', C.c_int64),
                ('l_slot', C.c_int64 * NUM_PARTS), ('l_nn', C.c_int64 * NUM_PARTS), ('l_w', C.c_int64 * NUM_PARTS),
                ('l_x', C.c_int64 * NUM_PARTS), ('l_d', C.c_int64 * NUM_PARTS), ('l_r', C.c_int64 * NUM_PARTS),
                ('emb', C.c_int64 * NUM_PARTS), ('occp', C.c_int64 * NUM_PARTS), ('wl', C.c_int64 * NUM_PARTS),
                ('wcnt', C.c_int64), ('wsel', C.c_int64), ('rgbw', C.c_int64), ('n_groups', C.c_int64), ('knn_dfar2', C.c_int64),
                ('byte_off', C.c_int64), ('dslice', C.c_int64), ('pdist', C.c_int64), ('feat', C.c_int64 * NUM_PARTS),
                ('gcount', C.c_int64)]


class InvrPerceptualLayout(C.Structure):
    """include/invr_perceptual.h: byte offsets of every intermediate of the perceptual loss in the caller's workspace."""
    ARRAYS = ('rank', 'img', 'a11', 'a12', 'pool', 'a21', 'a22', 'partial', 'out8', 'g22', 'gm22', 'g21', 'gm21', 'gpool', 'g12', 'gm12',
              'g11', 'gm11', 'gimg')
    _fields_ = [(k, C.c_int64) for k in ARRAYS + ('n_part1', 'n_part2', 'n_partial', 'bytes')]


class InvrImglossLayout(C.Structure):
    """include/invr_imgloss.h: byte offsets of every array of the SSIM / TV image terms in the caller's workspace."""
    ARRAYS = ('rank', 'img', 'mom', 'smap', 'pqr', 'occ', 'tvmax', 'partial', 'out8', 'gimg')
    _fields_ = [(k, C.c_int64) for k in ARRAYS + ('n_ssim', 'n_tv', 'n_partial', 'bytes')]


class InvrLpipsLayout(C.Structure):
    """include/invr_lpips.h: byte offsets of every stored array of the evaluator's LPIPS in the caller's workspace."""
    _fields_ = [('scaled', C.c_int64), ('act', C.c_int64 * 13), ('pool', C.c_int64 * 4), ('partial', C.c_int64), ('part_off', C.c_int64 * 5),
                ('n_part', C.c_int64 * 5), ('n_partial', C.c_int64), ('bytes', C.c_int64)]


class InvrMeshLayout(C.Structure):
    """include/invr_mesh.h: byte offsets of the per-point arrays of one surface extraction in the caller's workspace."""
    ARRAYS = ('masks', 'tcounts', 'voffsets', 'toffsets', 'counts', 'partials')
    _fields_ = [(k, C.c_int64) for k in ARRAYS + ('n_points', 'n_blocks', 'bytes')]


class InvrGeoOut(C.Structure):
    """include/invr_geomaps.h: the geometry outputs of invr_render_fwd_geo (NULL = not formed)."""
    _fields_ = [('level', C.c_float), ('depth_map', C.c_void_p), ('surf_index', C.c_void_p), ('surf_depth', C.c_void_p)]


def _signatures():
    """name -> (restype, argtypes) of every prototype of include/invr.h, in the header's order (tests/test_abi_symbols.py holds each
    entry against the header's text).  vp = any data pointer: device tensors, host arrays and the stream go through as addresses."""
    i32, i64, f32, f64, size, vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_void_p
    scene, model, grid = C.POINTER(InvrScene), C.POINTER(InvrModel), C.POINTER(InvrGrid)
    rays = [vp, vp, vp, vp, vp, i64, i32]          # ray_o, ray_d, near, far, jitter, n_rays, n_samples
    ws = [vp, size, i64, vp]                       # workspace, workspace_bytes, max_active, stream
    render = [scene, model] + rays + [vp, vp, vp, vp, vp, vp, vp] + ws
    return {
        'invr_last_error': (C.c_char_p, ()),
        'invr_version': (C.c_int, ()),
        'invr_sizeof': (size, [i32]),
        'invr_workspace_bytes': (size, [i64, i32, i64]),
        'invr_render_fwd': (C.c_int, render),
        'invr_raw_dirty_bytes': (size, [i64]),
        'invr_render_fwd_tracked': (C.c_int, render + [vp, i64]),
        'invr_geometry_fwd': (C.c_int, [scene, model] + rays + [vp, vp] + ws),
        'invr_field_workspace_bytes': (size, [i64, i64]),
        'invr_field_fwd': (C.c_int, [scene, model, vp, vp, i64, vp, vp, vp] + ws),
        'invr_workspace_layout': (C.c_int, [i64, i32, i64, C.POINTER(InvrWsLayout)]),
        'invr_profile_enable': (C.c_int, [i32]),
        'invr_profile_read': (C.c_int, [_f32p, _i32p]),
        'invr_grid_encode_fwd': (C.c_int, [grid, vp, i64, vp, vp]),
        'invr_grid_encode_bwd': (C.c_int, [grid, vp, vp, i64, vp, vp, vp, vp]),
        'invr_sample_volume': (C.c_int, [vp, i32 * 3, i32, i32, i32, vp, vp, i64, vp, vp]),
        'invr_knn_blend': (C.c_int, [scene, vp, i64, vp, vp, vp]),
        'invr_knn_neighbors': (C.c_int, [scene, vp, i64, vp, vp, vp, vp, vp]),
        'invr_pose_points': (C.c_int, [scene] + rays + [vp, i64, vp, vp, vp]),
        'invr_warp_deform': (C.c_int, [scene, model, vp, vp, vp, vp, i64, vp, vp, vp, vp]),
        'invr_part_field_workspace': (size, [i64]),
        'invr_part_field_fwd': (C.c_int, [model, i32, vp, vp, vp, i64, vp, vp, size, vp]),
        'invr_part_encode_workspace': (size, [i64]),
        'invr_part_encode_fwd': (C.c_int, [grid, vp, i64, i32, vp, vp, size, vp]),
        'invr_part_encode_fwd_all': (C.c_int, [grid, C.POINTER(vp), i64, vp, i64, i32, C.POINTER(vp), vp]),
        'invr_deform_fwd': (C.c_int, [scene, model, vp, i64, vp, vp]),
        'invr_distortion_fwd': (C.c_int, [vp, vp, i64, i32, vp, vp]),
        'invr_composite_fwd': (C.c_int, [vp, i64, i32, vp, vp, vp, vp]),
        'invr_generate_rays': (C.c_int, [_f64p, _f64p, _f64p, _f64p, _f32p, i32, i32, vp, vp, vp, vp, vp]),
        'invr_grid_row_sums_len': (i64, [vp]),
        'invr_grid_row_sums': (C.c_int, [vp, vp, vp]),
        'invr_part_mlp_fwd': (C.c_int, [model, i32, vp, vp, vp, i64, vp, vp, vp]),
        'invr_part_mlp_bwd': (C.c_int, [model, i32, vp, vp, vp, i64, vp, C.POINTER(InvrMlpBwdOut), vp]),
        'invr_adam_chunk_elems': (i32, ()),
        'invr_adam_advance': (C.c_int, [vp, i32, f64, f64, vp]),
        'invr_adam_step': (C.c_int, [vp, vp, vp, i64, f64, f64, f32, vp]),
        'invr_rigid_transformation': (C.c_int, [vp, vp, vp, vp, vp]),
        'invr_pack_parts': (C.c_int, [vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp]),
        'invr_train_workspace_bytes': (size, [i64, i32, i64]),
        'invr_train_fwd': (C.c_int, [scene, model] + rays + [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp] + ws),
        'invr_train_bwd': (C.c_int, [scene, model, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(InvrTrainGrads), i32] + ws),
        'invr_expand_row_grad': (C.c_int, [grid, vp, vp, vp, vp]),
        'invr_part_encode_bwd_lists': (C.c_int, [grid, vp, vp, i64, i64, vp, vp, vp, vp]),
        'invr_part_mlp_bwd_lists': (C.c_int, [model, i32, vp, vp, vp, i64, i64, vp, vp, vp, C.POINTER(InvrMlpBwdOut), i32, vp]),
        'invr_part_wgrad': (C.c_int, [vp, vp, i64, i32, C.POINTER(vp), C.POINTER(vp), vp, vp]),
        'invr_deform_bwd_list': (C.c_int, [scene, model, vp, vp, i64, vp, C.POINTER(InvrDeformBwdOut), C.POINTER(vp), C.POINTER(vp), vp, vp, vp]),
        'invr_distortion_bwd': (C.c_int, [vp, vp, vp, i64, i32, vp, vp]),
        'invr_train_loss_fwd': (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, i32, vp, vp, vp]),
        'invr_train_loss_bwd': (C.c_int, [vp, vp, vp, i64, f32, f32, f32, i32, vp, vp, vp, vp, vp]),
        'invr_merge_bwd': (C.c_int, [i32, vp, size, i64, i32, i64, vp, vp, vp]),
        'invr_composite_bwd': (C.c_int, [vp, vp, vp, vp, i64, i32, vp, vp]),
        'invr_eval_workspace_bytes': (size, [i32, i32]),
        'invr_image_assemble': (C.c_int, [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, size, vp]),
        'invr_image_metrics': (C.c_int, [vp, vp, i32, i32, i32, vp, vp, size, vp]),
    }


def _signatures_perceptual():
    """The same table for include/invr_perceptual.h (tests/test_abi_perceptual_cpu.py holds it against that header's text)."""
    i32, i64, f32, size, vp = C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_void_p
    ws = [vp, size]                                # workspace, workspace_bytes
    return {
        'invr_perceptual_packed_floats': (i64, ()),
        'invr_perceptual_pack_weights': (C.c_int, [C.POINTER(vp), C.POINTER(vp), vp, vp]),
        'invr_perceptual_workspace_bytes': (size, [i32, i32]),
        'invr_perceptual_workspace_layout': (C.c_int, [i32, i32, C.POINTER(InvrPerceptualLayout)]),
        'invr_perceptual_fwd': (C.c_int, [vp, vp, vp, vp, i64, i32, i32] + ws + [vp, vp]),
        'invr_perceptual_bwd': (C.c_int, [vp, vp, i64, i32, i32] + ws + [vp, vp, vp]),
        'invr_train_loss_lpips_fwd': (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i32, i32, f32, f32, f32, i32] + ws + [vp, vp, vp]),
        'invr_train_loss_lpips_bwd': (C.c_int, [vp, vp, vp, i64, i32, i32, f32, f32, f32, i32] + ws + [vp, vp, vp, vp, vp]),
    }


def _signatures_imgloss():
    """The same table for include/invr_imgloss.h (tests/test_abi_imgloss_cpu.py holds it against that header's text)."""
    i32, i64, f32, size, vp = C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_void_p
    ws = [vp, size]                                # workspace, workspace_bytes
    obj = [f32, f32, f32, i32]                     # w_pair, w_dist, w_off, use_pair
    return {
        'invr_imgloss_workspace_bytes': (size, [i32, i32, i32]),
        'invr_imgloss_workspace_layout': (C.c_int, [i32, i32, i32, C.POINTER(InvrImglossLayout)]),
        'invr_ssim_fwd': (C.c_int, [vp, vp, vp, vp, i32, i64, i32, i32] + ws + [vp, vp]),
        'invr_ssim_bwd': (C.c_int, [vp, vp, i32, i64, i32, i32] + ws + [vp, vp, vp]),
        'invr_tv_fwd': (C.c_int, [vp, vp, vp, vp, i64, i32, i32] + ws + [vp, vp]),
        'invr_tv_bwd': (C.c_int, [vp, i64, i32, i32] + ws + [vp, vp, vp]),
        'invr_train_loss_ssim_fwd': (C.c_int, [vp, vp, vp, vp, i32, vp, vp, i64, i32, i32] + obj + ws + [vp, vp, vp]),
        'invr_train_loss_ssim_bwd': (C.c_int, [vp, vp, i32, vp, i64, i32, i32] + obj + ws + [vp, vp, vp, vp, vp]),
        'invr_train_loss_tv_fwd': (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i32, i32] + obj + ws + [vp, vp, vp]),
        'invr_train_loss_tv_bwd': (C.c_int, [vp, vp, i64, i32, i32] + obj + ws + [vp, vp, vp, vp, vp]),
    }


def _signatures_lpips():
    """The same table for include/invr_lpips.h (tests/test_abi_lpips_cpu.py holds it against that header's text)."""
    i32, i64, size, vp = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p
    return {
        'invr_lpips_packed_floats': (i64, ()),
        'invr_lpips_pack_weights': (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp]),
        'invr_lpips_workspace_bytes': (size, [i32, i32, i32]),
        'invr_lpips_workspace_layout': (C.c_int, [i32, i32, i32, C.POINTER(InvrLpipsLayout)]),
        'invr_lpips_fwd': (C.c_int, [vp, vp, vp, i32, i32, i32, vp, size, vp, vp]),
    }


def _signatures_mesh():
    """The same table for include/invr_mesh.h (tests/test_abi_mesh_cpu.py holds it against that header's text)."""
    i32, i64, f32, size, vp = C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_void_p
    f3, i3 = f32 * 3, i32 * 3                       # origin / voxel / dims: host arrays
    return {
        'invr_grid_points': (C.c_int, [f3, f3, i3, i64, i64, vp, vp]),
        'invr_mesh_workspace_bytes': (size, [i3]),
        'invr_mesh_workspace_layout': (C.c_int, [i3, C.POINTER(InvrMeshLayout)]),
        'invr_mesh_count': (C.c_int, [vp, i3, f32, vp, size, vp, vp]),
        'invr_mesh_emit': (C.c_int, [vp, i3, f3, f3, f32, vp, size, vp, i64, vp, i64, vp, vp]),
    }


def _signatures_batch():
    """The same table for include/invr_batch.h (tests/test_abi_batch_cpu.py holds it against that header's text)."""
    i32, vp = C.c_int32, C.c_void_p
    return {
        'invr_patch_batch': (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, _f32p, _f64p, _f64p, _f64p, _f32p, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    }


def _signatures_sample():
    """The same table for include/invr_sample.h (tests/test_abi_sample_cpu.py holds it against that header's text)."""
    i32, vp = C.c_int32, C.c_void_p
    return {
        'invr_ray_batch': (C.c_int, [vp, vp, vp, vp, i32, i32, vp, i32, _f64p, _f64p, _f64p, _f64p, _f32p, vp, vp, vp, vp, vp, vp, vp]),
    }


def _signatures_vertex():
    """The same table for include/invr_vertex.h (tests/test_abi_vertex_sums_cpu.py holds it against that header's text)."""
    i64, vp = C.c_int64, C.c_void_p
    return {
        'invr_grid_vertex_sums_len': (i64, [vp, i64]),
        'invr_grid_vertex_sums': (C.c_int, [vp, i64, vp, vp]),
    }


def _signatures_posescene():
    """The same table for include/invr_posescene.h (tests/test_abi_posescene_cpu.py holds it against that header's text)."""
    i32, size, vp = C.c_int32, C.c_size_t, C.c_void_p
    d3, i3 = C.c_double * 3, i32 * 3                # origin / step / dims: host arrays
    return {
        'invr_distance_volume_workspace_bytes': (size, [i32]),
        'invr_distance_volume': (C.c_int, [vp, i32, d3, d3, i3, vp, vp, vp, size, vp]),
    }


def _signatures_surface():
    """The same table for include/invr_surface.h (tests/test_abi_surface_cpu.py holds it against that header's text)."""
    i32, i64, size, vp = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p
    d3, i3 = C.c_double * 3, i32 * 3                # origin / step / dims: host arrays
    return {
        'invr_surface_volume_workspace_bytes': (size, [i32]),
        'invr_surface_volume': (C.c_int, [vp, i32, vp, i32, d3, d3, i3, vp, vp, vp, vp, size, vp]),
        'invr_surface_interpolate': (C.c_int, [vp, i32, i32, vp, i32, vp, vp, i64, vp, i64, i64, vp]),
    }


def _signatures_geomaps():
    """The same table for include/invr_geomaps.h (tests/test_geomaps_abi_cpu.py holds it against that header's text)."""
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    return {
        'invr_depth_fwd': (C.c_int, [vp, vp, vp, vp, i64, i32, f32, f32, vp, vp, vp, vp]),
        'invr_render_fwd_geo': (C.c_int, SIGNATURES['invr_render_fwd_tracked'][1] + [C.POINTER(InvrGeoOut)]),
        'invr_surface_stencil': (C.c_int, [vp, vp, vp, vp, i64, f32, vp, vp, vp]),
        'invr_stencil_normals': (C.c_int, [vp, vp, i64, vp, vp, vp]),
    }


SIGNATURES = _signatures()
SIGNATURES_VERTEX = _signatures_vertex()
SIGNATURES_PERCEPTUAL = _signatures_perceptual()
SIGNATURES_IMGLOSS = _signatures_imgloss()
SIGNATURES_LPIPS = _signatures_lpips()
SIGNATURES_MESH = _signatures_mesh()
SIGNATURES_BATCH = _signatures_batch()
SIGNATURES_SAMPLE = _signatures_sample()
SIGNATURES_POSESCENE = _signatures_posescene()
SIGNATURES_SURFACE = _signatures_surface()
SIGNATURES_GEOMAPS = _signatures_geomaps()
SIZEOF_GEO_OUT = 10      # include/invr_geomaps.h INVR_SIZEOF_GEO_OUT
EXPORTS = list(SIGNATURES)
ABI_VERSION = 2          # include/invr.h INVR_ABI_VERSION
BWD_HEAD, BWD_DEFORMER, BWD_ALL = 1, 64, 127
EVAL_RESULT_BYTES = 64   # include/invr.h INVR_EVAL_RESULT_BYTES: float64[3] (SSE, sum gt, sum S), int32[8] (windows, x, y, w, h, status, set, 0)
NUM_STAGES = 14
STAGE_NAMES = ['cull', 'knn', 'warp'] + ['encode_%d' % p for p in range(5)] + ['mlp_%d' % p for p in range(5)] + ['composite']

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libinvr.so is not built (%s); run `python -c "import __graft_entry__ as g; g.build()"`. '
                               'There is no CPU fallback for the render path.' % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in (list(SIGNATURES.items()) + list(SIGNATURES_PERCEPTUAL.items()) + list(SIGNATURES_IMGLOSS.items())
                                          + list(SIGNATURES_LPIPS.items())
                                          + list(SIGNATURES_MESH.items())
                                          + list(SIGNATURES_BATCH.items()) + list(SIGNATURES_SAMPLE.items()) + list(SIGNATURES_VERTEX.items())
                                          + list(SIGNATURES_POSESCENE.items()) + list(SIGNATURES_SURFACE.items())
                                          + list(SIGNATURES_GEOMAPS.items())):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        if L.invr_version() != ABI_VERSION:
            raise RuntimeError('libinvr.so speaks ABI version %d, this binding %d (include/invr.h INVR_ABI_VERSION): rebuild the library '
                               '(python -m invr.build)' % (L.invr_version(), ABI_VERSION))
        for i, t in enumerate((InvrGrid, InvrMlp, InvrPart, InvrModel, InvrScene, InvrWsLayout, InvrMlpBwdOut, InvrAdamTensor, InvrTrainGrads,
                               InvrDeformBwdOut, InvrGeoOut)):
            if L.invr_sizeof(i) != C.sizeof(t):
                raise RuntimeError('libinvr ABI mismatch: struct %s is %d bytes in the library, %d in the binding'
                                   % (t.__name__, L.invr_sizeof(i), C.sizeof(t)))
        _lib = L
    return _lib


def profile_enable(on):
    lib().invr_profile_enable(int(bool(on)))


def profile_read():
    """-> ({stage name: total ms since the last read}, number of renders)."""
    ms = (C.c_float * NUM_STAGES)()
    n = C.c_int32(0)
    check(lib().invr_profile_read(ms, C.byref(n)))
    return {STAGE_NAMES[i]: float(ms[i]) for i in range(NUM_STAGES)}, int(n.value)


def check(status):
    if status != 0:
        raise RuntimeError('libinvr: ' + lib().invr_last_error().decode())


def ws_views(ws, n_rays, S, max_active, n_active=None):
    """Zero-copy tensor views of the arrays invr_render_fwd left in the workspace `ws` (uint8 tensor)."""
    lay = InvrWsLayout()
    check(lib().invr_workspace_layout(n_rays, S, max_active, C.byref(lay)))
    lc = lay.lcap

    def view(off, count, dtype):
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return ws[off:off + nbytes].view(dtype)
    v = {'cap': lay.cap, 'lcap': lc,
         'counters': view(lay.counters, 16, torch.int32),
         'active_idx': view(lay.active_idx, lc, torch.int32),
         'word_off': view(lay.word_off, (n_rays * S + 1023) // 1024 * 16, torch.int32),
         'mask': view(lay.mask, (n_rays * S + 1023) // 1024 * 16, torch.int64),
         'byte_off': view(lay.byte_off, (n_rays * S + 1023) // 1024 * 128, torch.int32),        # (eval frames: depth-windowed order)
         'pflags': view(lay.pflags, lc, torch.uint8), 'farflags': view(lay.farflags, lc, torch.uint8),
         'knn_dfar2': view(lay.knn_dfar2, 1, torch.float32),
         'dslice': view(lay.dslice, DF_SLICE_MAX * 2, torch.float32).view(DF_SLICE_MAX, 2),     # per-frame (u, v) slices of the deformer grid
         'wsel': view(lay.wsel, lc, torch.uint8),                   # merge result per survivor (p / 8 + p / 255)
         'rgbw': view(lay.rgbw, (lc + 8) * 4, torch.float32).view(lc + 8, 4),      # winner's [rgb, occ] per slot; far constants at lc + p
         'wcnt': view(lay.wcnt, lay.n_groups * NUM_PARTS, torch.int32).view(lay.n_groups, NUM_PARTS)}
    v['pdist'] = view(lay.pdist, lc * NUM_PARTS, torch.float32).view(lc, NUM_PARTS)      # part_dist per (slot, part): aggr 'dist' / 'mindist' frames
    v['gcount'] = view(lay.gcount, lay.n_groups * NUM_PARTS, torch.int32).view(lay.n_groups, NUM_PARTS)
    v['feat'] = [view(lay.feat[p], lc * 16, torch.float32).view(lc * 4, 4) for p in range(NUM_PARTS)]      # 'mean' / 'dist': row pair * 4 = the pair's [rgb, occ]
    v['occp'] = [view(lay.occp[p], lc, torch.float32) for p in range(NUM_PARTS)]      # occupancy of every listed pair
    v['wl'] = [view(lay.wl[p], lc, torch.int32) for p in range(NUM_PARTS)]
    for k in ('l_slot', 'l_x', 'l_d', 'l_r'):
        offs = getattr(lay, k)
        if k == 'l_slot':
            v[k] = [view(offs[p], lc, torch.int32) for p in range(NUM_PARTS)]
        else:
            v[k] = [view(offs[p], 3 * lc, torch.float32).view(3, lc) for p in range(NUM_PARTS)]
    v['l_nn'] = [view(lay.l_nn[p], 4 * lc, torch.int32).view(lc, 4) for p in range(NUM_PARTS)]      # neighbour rows inside part_pts[p]
    v['l_w'] = [view(lay.l_w[p], 4 * lc, torch.float32).view(lc, 4) for p in range(NUM_PARTS)]       # normalised gaussian weights
    v['emb'] = [view(lay.emb[p], 20 * lc, torch.float32).view(20, lc) for p in range(NUM_PARTS)]      # encoder outputs, SoA [k][pair]
    return v


def perceptual_views(ws, H, W):
    """Zero-copy tensor views of every array invr_perceptual_fwd / _bwd keep in the workspace `ws` (uint8 tensor): the assembled images,
    the stored activations of both images, the per-wave partial sums and the gradient arriving at each layer's output."""
    lay = InvrPerceptualLayout()
    check(lib().invr_perceptual_workspace_layout(H, W, C.byref(lay)))
    P, h, w = H * W, H // 2, W // 2

    def view(off, shape, dtype=torch.float32):
        count = 1
        for d in shape:
            count *= d
        return ws[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
    v = {'layout': lay, 'rank': view(lay.rank, (H, W), torch.int32), 'img': view(lay.img, (2, 3, H, W)),
         'a11': view(lay.a11, (2, 64, H, W)), 'a12': view(lay.a12, (2, 64, H, W)), 'pool': view(lay.pool, (2, 64, h, w)),
         'a21': view(lay.a21, (2, 128, h, w)), 'a22': view(lay.a22, (2, 128, h, w)),
         'partial': view(lay.partial, (lay.n_partial,), torch.float64), 'out8': view(lay.out8, (8,)),
         'gpool': view(lay.gpool, (64, h, w)), 'gimg': view(lay.gimg, (3, H, W))}
    for k in ('g22', 'gm22', 'g21', 'gm21'):
        v[k] = view(getattr(lay, k), (128, h, w))
    for k in ('g12', 'gm12', 'g11', 'gm11'):
        v[k] = view(getattr(lay, k), (64, H, W))
    return v


def imgloss_views(ws, H, W, window=11):
    """Zero-copy tensor views of every array the SSIM / TV image terms keep in the workspace `ws` (uint8 tensor): the assembled images,
    the five filtered maps, S, p / q / r, mask_gt, the partial sums and the gradient of the assembled predicted image."""
    lay = InvrImglossLayout()
    check(lib().invr_imgloss_workspace_layout(H, W, window, C.byref(lay)))

    def view(off, shape, dtype=torch.float32):
        count = 1
        for d in shape:
            count *= d
        return ws[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
    return {'layout': lay, 'rank': view(lay.rank, (H, W), torch.int32), 'img': view(lay.img, (2, 3, H, W)), 'mom': view(lay.mom, (5, 3, H, W)),
            'smap': view(lay.smap, (3, H, W)), 'pqr': view(lay.pqr, (3, 3, H, W)), 'occ': view(lay.occ, (H, W), torch.uint8),
            'tvmax': view(lay.tvmax, (2, lay.n_tv)), 'partial': view(lay.partial, (lay.n_partial,), torch.float64),
            'out8': view(lay.out8, (8,)), 'gimg': view(lay.gimg, (3, H, W))}


LPIPS_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
LPIPS_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_BLOCK = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)          # layer -> block: its map is (H >> block) x (W >> block)
LPIPS_TAPS = (1, 3, 6, 9, 12)                                   # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3


def lpips_views(ws, H, W):
    """Zero-copy tensor views of every array invr_lpips_fwd(keep = 1) leaves in the workspace `ws` (uint8 tensor): the scaled planar
    input, the 13 activations, the 4 pooled maps and the partial sums (16 pixels each) of each tap."""
    lay = InvrLpipsLayout()
    check(lib().invr_lpips_workspace_layout(H, W, 1, C.byref(lay)))

    def view(off, shape, dtype=torch.float32):
        count = 1
        for d in shape:
            count *= d
        return ws[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
    v = {'layout': lay, 'scaled': view(lay.scaled, (2, 3, H, W)),
         'act': [view(lay.act[l], (2, LPIPS_COUT[l], H >> LPIPS_BLOCK[l], W >> LPIPS_BLOCK[l])) for l in range(13)],
         'pool': [view(lay.pool[b], (2, LPIPS_CIN[LPIPS_TAPS[b] + 1], H >> (b + 1), W >> (b + 1))) for b in range(4)],
         'partial': [view(lay.partial + 8 * lay.part_off[t], (lay.n_part[t],), torch.float64) for t in range(5)]}
    return v


def lpips_pack(conv_w, conv_b, lin_w, shift, scale, packed=None):
    """The packed weight image of invr_lpips_pack_weights from the 13 (out, in, 3, 3) weights, (out) biases, the five lin vectors (C)
    and the scaling layer's shift / scale (3) — device tensors."""
    L = lib()
    ws, bs, ls = [f32c(t) for t in conv_w], [f32c(t) for t in conv_b], [f32c(t).reshape(-1) for t in lin_w]
    assert [tuple(t.shape) for t in ws] == [(o, i, 3, 3) for i, o in zip(LPIPS_CIN, LPIPS_COUT)], [tuple(t.shape) for t in ws]
    assert [tuple(t.shape) for t in bs] == [(o,) for o in LPIPS_COUT], [tuple(t.shape) for t in bs]
    assert [tuple(t.shape) for t in ls] == [(LPIPS_COUT[l],) for l in LPIPS_TAPS], [tuple(t.shape) for t in ls]
    sh, sc = f32c(shift).reshape(-1), f32c(scale).reshape(-1)
    assert sh.numel() == 3 and sc.numel() == 3
    if packed is None:
        packed = torch.empty(L.invr_lpips_packed_floats(), device=ws[0].device)
    arr = lambda ts: (C.c_void_p * len(ts))(*[ptr(t).value for t in ts])
    check(L.invr_lpips_pack_weights(arr(ws), arr(bs), arr(ls), ptr(sh), ptr(sc), ptr(packed), stream_ptr()))
    return packed


def mesh_views(ws, dims):
    """Zero-copy tensor views of the arrays invr_mesh_count keeps in the workspace `ws` (uint8 tensor) for a volume of `dims`."""
    lay = InvrMeshLayout()
    check(lib().invr_mesh_workspace_layout((C.c_int32 * 3)(*dims), C.byref(lay)))
    n, nb = lay.n_points, lay.n_blocks
    return {'layout': lay, 'masks': ws[lay.masks:lay.masks + n], 'tcounts': ws[lay.tcounts:lay.tcounts + n],
            'voffsets': ws[lay.voffsets:lay.voffsets + 4 * n].view(torch.int32), 'toffsets': ws[lay.toffsets:lay.toffsets + 4 * n].view(torch.int32),
            'counts': ws[lay.counts:lay.counts + 32].view(torch.int64),
            'partials': ws[lay.partials:lay.partials + 8 * nb].view(torch.int32).view(2, nb)}


def perceptual_pack(weights, biases, packed=None):
    """The packed weight image of invr_perceptual_pack_weights from the four (out, in, 3, 3) weights and (out) biases (device tensors)."""
    L = lib()
    ws = [f32c(t) for t in weights]
    bs = [f32c(t) for t in biases]
    assert [tuple(t.shape) for t in ws] == [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3)], [tuple(t.shape) for t in ws]
    assert [tuple(t.shape) for t in bs] == [(64,), (64,), (128,), (128,)]
    if packed is None:
        packed = torch.empty(L.invr_perceptual_packed_floats(), device=ws[0].device)
    wp = (C.c_void_p * 4)(*[ptr(t).value for t in ws])
    bp = (C.c_void_p * 4)(*[ptr(t).value for t in bs])
    check(L.invr_perceptual_pack_weights(wp, bp, ptr(packed), stream_ptr()))
    return packed


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t, dtype=torch.float32):
    """Device pointer of a contiguous CUDA tensor of the expected dtype (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda, 'libinvr needs device tensors (got a CPU tensor)'
    assert t.dtype == dtype, (t.dtype, dtype)
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def f32c(t):
    """What ptr() asks for: the detached, fp32, contiguous form of a tensor (itself where it already is that)."""
    return t.detach().to(torch.float32).contiguous()


def make_grid(spec, dense, hsh, bounds, keep):
    """InvrGrid from params.grid_spec(...) + table tensors.  `keep` collects tensors to keep alive."""
    g = InvrGrid()
    hsh = f32c(hsh); keep.append(hsh)
    g.hash = hsh.data_ptr()
    if dense is not None:
        dense = f32c(dense); keep.append(dense)
        g.dense = dense.data_ptr()
    bounds = f32c(bounds); keep.append(bounds)
    g.bounds = bounds.data_ptr()
    g.n_levels, g.n_features, g.start_hash = spec['L'], spec['F'], spec['start_hash']
    g.separate_dense, g.table_len = int(spec['separate_dense']), spec['T']
    for l in range(spec['L']):
        g.res[l] = spec['res'][l]
        g.cell[l] = float(spec['size'][l])
        g.dense_off[l] = spec['dense_off'][l]
    g.sum, g.sum_over_features, g.include_input = int(spec['sum']), int(spec['sum_over_features']), int(spec['include_input'])
    return g


def make_mlp(weights, biases, keep):
    m = InvrMlp()
    m.n_linear = len(weights)
    for i, (w, b) in enumerate(zip(weights, biases)):
        w, b = f32c(w), f32c(b)
        keep += [w, b]
        m.weight[i], m.bias[i] = w.data_ptr(), b.data_ptr()
        m.dims[i], m.dims[i + 1] = w.shape[1], w.shape[0]
    return m


def make_model(sd, cfg, keep):
    """InvrModel from a reference-keyed state_dict of device tensors."""
    m = InvrModel()
    dspec = params.deformer_grid_spec(cfg)
    p = 'tpose_deformer.embedder.'
    m.deform_grid = make_grid(dspec, sd.get(p + 'dense'), sd[p + 'hash'], sd[p + 'bounds'], keep)
    m.deform_mlp = make_mlp([sd['tpose_deformer.mlp.%d.weight' % k] for k in (0, 2, 4)],
                            [sd['tpose_deformer.mlp.%d.bias' % k] for k in (0, 2, 4)], keep)
    for i, name in enumerate(PART_NAMES):
        q = 'tpose_human.part_networks.%d.' % i
        spec = params.part_grid_spec(cfg, name)
        part = m.part[i]
        part.grid = make_grid(spec, sd.get(q + 'embedder.dense'), sd[q + 'embedder.hash'], sd[q + 'embedder.bounds'], keep)
        occ_dims, rgb_dims = params.mlp_dims(cfg, name)
        part.occ = make_mlp([sd[q + 'occ.linears.%d.weight' % k] for k in range(len(occ_dims) - 1)],
                            [sd[q + 'occ.linears.%d.bias' % k] for k in range(len(occ_dims) - 1)], keep)
        part.rgb = make_mlp([sd[q + 'rgb.linears.%d.weight' % k] for k in range(len(rgb_dims) - 1)],
                            [sd[q + 'rgb.linears.%d.bias' % k] for k in range(len(rgb_dims) - 1)], keep)
        lat = f32c(sd[q + 'rgb_latent']); keep.append(lat)
        part.rgb_latent = lat.data_ptr()
        part.latent_dim, part.num_latent_code = lat.shape[1], lat.shape[0]
    m.n_dir_freq = cfg.viewdir_embedder.kwargs['res']
    m.geo_feature_dim = cfg.geo_feature_dim
    return m


def make_scene(batch, cfg, keep):
    """InvrScene from the reference's collated batch dict (device tensors, leading dim 1)."""
    s = InvrScene()

    def f(k):
        t = f32c(batch[k][0]); keep.append(t)
        return t
    s.R, s.Th, s.A, s.big_A = f('R').data_ptr(), f('Th').data_ptr(), f('A').data_ptr(), f('big_A').data_ptr()
    pbw, tuv = f('pbw'), f('tuv')
    s.pbw, s.tuv = pbw.data_ptr(), tuv.data_ptr()
    for a in range(3):
        s.pbw_dims[a], s.tuv_dims[a] = pbw.shape[a], tuv.shape[a]
    s.pbw_channels = pbw.shape[3]
    assert tuv.shape[3] == 2
    s.pbounds, s.tbounds = f('pbounds').data_ptr(), f('tbounds').data_ptr()
    pp, pb = f('part_pts'), f('part_pbw')
    assert pp.shape[0] == NUM_PARTS and pb.shape[2] == 24
    s.part_pts, s.part_pbw, s.part_stride = pp.data_ptr(), pb.data_ptr(), pp.shape[1]
    l2 = batch['lengths2'][0].to(torch.int64).contiguous(); keep.append(l2)
    s.lengths2 = l2.data_ptr()
    fd = batch['frame_dim'].reshape(-1)[:1].to(torch.float32).contiguous(); keep.append(fd)
    li = batch['latent_index'].reshape(-1)[:1].to(torch.int64).contiguous(); keep.append(li)
    s.frame_dim, s.latent_index = fd.data_ptr(), li.data_ptr()
    s.smpl_thresh, s.tpose_viewdir = float(cfg.smpl_thresh), int(bool(cfg.tpose_viewdir))
    s.aggr = {'': 0, 'mean': 1, 'dist': 2, 'mindist': 3}[cfg.get('aggr', '') or '']          # inb_part_network_multiassign.py:236-256 (INVR_AGGR_*)
    s.composite_eps = float(bool(cfg.get('random_bg', False)))          # inb_renderer.py:72 passes cfg.random_bg as render_weights' epsilon
    return s
