"""ctypes binding of libhistogan_hip.so (the C ABI declared in include/hg_hist.h).

There is deliberately NO fallback: if the library is missing or fails to load,
importing this module raises, and every op built on it is unusable.
"""
import ctypes
import os

import torch  # before the library is loaded, so that libamdhip64.so.7 resolves to the runtime torch uses

_PKG = os.path.dirname(os.path.abspath(__file__))
_TAG = os.environ.get('HG_LIB_TAG', '')  # experiment builds only (histogan_amd/build.py)
LIB_PATH = os.path.join(_PKG, 'libhistogan_hip' + ('_' + _TAG if _TAG else '') + '.so')

HG_METHOD = {'thresholding': 0, 'RBF': 1, 'inverse-quadratic': 2}
HG_RESIZE_NONE, HG_RESIZE_BILINEAR, HG_RESIZE_SAMPLING = 0, 1, 2
HG_PROJ = {'rgbuv': 0, 'rgchroma': 1, 'direct': 2, 'lab': 3}
# hg_hist_route.fwd / .bwd (the HG_ROUTE_FWD_* / HG_ROUTE_BWD_* enums of include/hg_hist.h), by value
HG_ROUTE_FWD = ('DENSE', 'THR_SCATTER', 'THR_LEAN', 'RBF_SCATTER')
# hg_conv_route.kind / .tile (the HG_CONV_* enums of include/hg_conv.h), by value
HG_CONV_KIND = ('SINGLE', 'PARITY4', 'PER_CLASS')
HG_CONV_TILE = ('16x256', '32x256', '64x256', '128x128', '128x128_SM', '64x64')
HG_ROUTE_BWD = ('MIRRORED', 'PLANES', 'GENERIC', 'THR_GATHER', 'RBF_GATHER', 'THR_LEAN', 'ZERO')


class HgHistParams(ctypes.Structure):
    """struct hg_hist_params (include/hg_hist.h)."""
    _fields_ = [
        ('struct_size', ctypes.c_uint32),
        ('B', ctypes.c_int32), ('C', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
        ('stride_b', ctypes.c_int64), ('stride_c', ctypes.c_int64),
        ('stride_h', ctypes.c_int64), ('stride_w', ctypes.c_int64),
        ('Hs', ctypes.c_int32), ('Ws', ctypes.c_int32),
        ('resize_mode', ctypes.c_int32),
        ('row_idx', ctypes.c_void_p), ('col_idx', ctypes.c_void_p),
        ('h', ctypes.c_int32),
        ('lo', ctypes.c_double), ('hi', ctypes.c_double),
        ('method', ctypes.c_int32),
        ('sigma', ctypes.c_double),
        ('intensity_scale', ctypes.c_int32),
        ('green_only', ctypes.c_int32),
        ('projection', ctypes.c_int32),
        ('pre_relu', ctypes.c_int32),
        ('proj_cache', ctypes.c_void_p),
        ('weight', ctypes.c_void_p),
        ('weight_stride_b', ctypes.c_int64), ('weight_stride_h', ctypes.c_int64), ('weight_stride_w', ctypes.c_int64),
    ]


class HgHistRoute(ctypes.Structure):
    """struct hg_hist_route (include/hg_hist.h): what hg_rgbuv_hist_route fills in."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'fwd', 'bwd', 'fwd_slices', 'bwd_workgroups', 'planes_rt',
                                              'rbf_radius', 'uses_proj_cache')]


class HgConvQuery(ctypes.Structure):
    """struct hg_conv_query (include/hg_conv.h): the call hg_conv2d_route is asked about."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'dgrad', 'B', 'K', 'N', 'Hi', 'Wi', 'ksize', 'stride', 'fe',
                                              'have_workspace')] + [('workspace_bytes', ctypes.c_size_t)]


class HgConvRoute(ctypes.Structure):
    """struct hg_conv_route (include/hg_conv.h): what hg_conv2d_route fills in."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'kind', 'tile', 'kchunk', 'ksplit', 'reduce', 'cus')] + \
               [('blocks', ctypes.c_int64), ('slab_bytes', ctypes.c_size_t)]


class HgWinoQuery(ctypes.Structure):
    """struct hg_wino_query (include/hg_wino.h): the call hg_wino_route / hg_wino_wgrad_route is asked about."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'B', 'K', 'N', 'H', 'W', 'fe', 'have_workspace')] + \
               [('workspace_bytes', ctypes.c_size_t)]


class HgWinoRoute(ctypes.Structure):
    """struct hg_wino_plan (include/hg_wino.h): what hg_wino_route fills in."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'variant', 'fe', 'nblk', 'nch', 'lTW', 'lTH', 'lNI', 'bt_x', 'bt_y',
                                              'blocks', 'ksplit', 'chunks_per_split', 'last_split_chunks', 'empty_splits', 'xcd',
                                              'grid', 'persistent', 'reduce', 'cus', 'supported', 'reserved')] + \
               [('slab_bytes', ctypes.c_size_t)]


class HgWinoWgradRoute(ctypes.Structure):
    """struct hg_wino_wgrad_plan (include/hg_wino.h): what hg_wino_wgrad_route fills in."""
    _fields_ = [(n, ctypes.c_int32) for n in ('struct_size', 'lPW', 'lPH', 'lPI', 'lcg', 'lrg', 'nchunks', 'ktiles', 'ntiles',
                                              'splits', 'chunks_per_split', 'last_split_chunks', 'empty_splits', 'reduce_groups',
                                              'xcd', 'grid', 'persistent', 'cus', 'supported', 'reserved')] + \
               [('slab_bytes', ctypes.c_size_t)]


class GlinLayer(ctypes.Structure):
    """struct hg_glin_layer (include/hg_linear.h)."""
    _fields_ = [('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('b', ctypes.c_void_p), ('y', ctypes.c_void_p),
                ('gw', ctypes.c_void_p), ('gb', ctypes.c_void_p), ('N', ctypes.c_int32), ('group', ctypes.c_int32)]


class HgDataItem(ctypes.Structure):
    """struct hg_data_item (include/hg_data.h); histogan_amd.data lays the same 56 bytes out as a numpy record."""
    _fields_ = [('src', ctypes.c_uint64), ('dst', ctypes.c_uint64), ('src_stride', ctypes.c_int64), ('dst_stride', ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ('n_out', 'n_keep', 'tab_off', 'in_base', 'in_len', 'flags')]


def _signatures():
    """name -> (restype, [argtypes]) of every symbol the headers under include/ declare, grouped by header.  _load applies it
    and EXPORTS is its keys: tests/test_cabi_cpu.py holds it against the prototypes."""
    ci, vp, sz, i32, i64, f32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    f64 = ctypes.c_double
    P = ctypes.POINTER
    PP, GL = P(HgHistParams), P(GlinLayer)
    return {
        # include/hg_hist.h
        'hg_version': (ci, []),
        'hg_error_string': (ctypes.c_char_p, [ci]),
        'hg_rgbuv_hist_workspace_bytes': (ci, [PP, P(sz), P(sz)]),
        'hg_rgbuv_hist_uses_proj_cache': (ci, [PP]),
        'hg_rgbuv_hist_route': (ci, [PP, ci, P(HgHistRoute)]),
        'hg_rgbuv_hist_fwd': (ci, [PP, vp, vp, vp, vp, sz, vp]),
        'hg_rgbuv_hist_bwd': (ci, [PP, vp, vp, vp, vp, vp, vp, sz, vp]),
        'hg_rgbuv_hist_bwd_w_workspace_bytes': (ci, [PP, P(sz)]),
        'hg_rgbuv_hist_bwd_w': (ci, [PP, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        'hg_hellinger_workspace_bytes': (sz, [i64]),
        'hg_hellinger_fwd_bwd': (ci, [vp, vp, i64, i32, f32, vp, vp, vp, sz, vp]),
        'hg_selftest_fastlog': (ci, [vp, vp]),
        # include/hg_nets.h
        'hg_modulate_fwd': (ci, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        'hg_modulate_bwd': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_nets_workspace_bytes': (sz, [i32, i32, i32, i32]),
        'hg_torgb_fwd': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        'hg_torgb_bwd_workspace_bytes': (sz, [i32, i32, i32, i32]),
        'hg_torgb_bwd': (ci, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        'hg_gstage_bwd_workspace_bytes': (sz, [i32, i32, i32, i32]),
        'hg_gstage_bwd': (ci, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32,
                               i32, vp, sz, vp]),
        'hg_channel_sum': (ci, [vp, vp, i32, i32, i32, vp, sz, vp]),
        'hg_demod_noise_lrelu_fwd': (ci, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        'hg_demod_noise_lrelu_bwd': (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        'hg_noise_grad': (ci, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        'hg_lrelu_bwd_channel_sum': (ci, [vp, vp, f32, vp, vp, i32, i32, i32, vp, sz, vp]),
        'hg_demod_style_grad_workspace_bytes': (sz, [i32, i32, i32]),
        'hg_demod_style_grad': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
        'hg_demod_weight_term': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        'hg_diffgrad_step': (ci, [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, vp]),
        'hg_diffgrad_step_size': (f32, [f32, f32, f32, i32]),
        'hg_diffgrad_step_dev': (ci, [vp, vp, vp, vp, vp, i64, vp, f32, f32, f32, vp]),
        'hg_ema_update': (ci, [vp, vp, i64, f32, vp]),
        # include/hg_conv.h
        'hg_conv_packed_elems': (sz, [i32, i32, i32, i32]),
        'hg_conv_pack_weights': (ci, [vp, vp, i32, i32, i32, i32, vp]),
        'hg_conv_pack_weights_both': (ci, [vp, vp, vp, i32, i32, i32, vp]),
        'hg_conv2d_fwd': (ci, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_conv2d_fwd_add': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_modconv2d_fwd': (ci, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_conv2d_workspace_bytes': (sz, [i32, i32, i32, i32, i32, i32, i32, i32]),
        'hg_conv_pack_blocks': (i32, [i32, i32]),
        'hg_conv_pack_weights_multi': (ci, [vp, i32, i32, vp]),
        'hg_conv2d_plan': (ci, [i32, i32, i32, i32, i32, i32, i32, i32, P(i32)]),
        'hg_conv2d_route': (ci, [P(HgConvQuery), P(HgConvRoute)]),
        'hg_conv2d_dgrad': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_conv2d_wgrad_workspace_bytes': (sz, [i32, i32, i32, i32, i32, i32, i32]),
        'hg_conv2d_wgrad': (ci, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
        # include/hg_recolor.h
        'hg_instnorm_workspace_bytes': (sz, [i64]),
        'hg_instnorm_lrelu_fwd': (ci, [vp, vp, vp, i64, i32, f32, f32, vp, sz, vp]),
        'hg_instnorm_lrelu_bwd': (ci, [vp, vp, vp, vp, i64, i32, f32, vp, sz, vp]),
        'hg_stencil3': (ci, [vp, vp, P(f32), i32, i32, i32, i32, i32, vp]),
        'hg_depthwise_valid': (ci, [vp, vp, vp, i64, i32, i32, i32, i32, vp]),
        # include/hg_linear.h
        'hg_grouped_linear_fwd': (ci, [GL, i32, i32, i32, vp]),
        'hg_grouped_linear_bwd_input_workspace_bytes': (sz, [GL, i32, i32, i32]),
        'hg_grouped_linear_bwd_input': (ci, [GL, i32, P(vp), i32, i32, i32, vp, sz, vp]),
        'hg_grouped_linear_bwd_params': (ci, [GL, i32, i32, i32, vp]),
        # include/hg_wino.h
        'hg_wino_supported': (ci, [i32, i32, i32, i32, i32]),
        'hg_wino_packed_elems': (sz, [i32, i32, i32]),
        'hg_wino_pack_weights': (ci, [vp, vp, i32, i32, i32, vp]),
        'hg_wino_pack_blocks': (i32, [i32, i32, i32, i32]),
        'hg_wino_pack_weights_multi': (ci, [vp, i32, i32, vp]),
        'hg_wino_workspace_bytes': (sz, [i32, i32, i32, i32, i32]),
        'hg_wino_conv2d': (ci, [vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_wino_wgrad_supported': (ci, [i32, i32, i32, i32, i32]),
        'hg_wino_wgrad_workspace_bytes': (sz, [i32, i32, i32, i32, i32]),
        'hg_wino_wgrad': (ci, [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        'hg_wino_route': (ci, [P(HgWinoQuery), P(HgWinoRoute)]),
        'hg_wino_wgrad_route': (ci, [P(HgWinoQuery), P(HgWinoWgradRoute)]),
        # include/hg_augment.h
        'hg_augment_spatial': (ci, [vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        'hg_augment_workspace_bytes': (sz, [i32]),
        'hg_sample_mean': (ci, [vp, vp, i32, i64, vp, sz, vp]),
        'hg_augment_color': (ci, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        # include/hg_post.h
        'hg_resize_axis': (ci, [vp, i32, i64, i64, i64, i32, vp, i32, i64, i64, i64, i32, i32, i32, i32, vp, vp, i32, i32,
                                vp]),
        'hg_pyr_down': (ci, [vp, vp, i32, i32, i32, vp]),
        'hg_pyr_up_add': (ci, [vp, vp, vp, f32, vp, vp, f32, vp, i32, i32, i32, vp]),
        'hg_color_moments_workspace_bytes': (sz, [i64]),
        'hg_color_moments': (ci, [vp, i64, i64, i64, vp, vp, sz, vp]),
        'hg_color_affine': (ci, [vp, i64, i64, i64, P(f32), vp, i32, vp]),
        'hg_u8_hwc_to_f32': (ci, [vp, vp, i32, i64, vp]),
        'hg_f32_to_u8_hwc': (ci, [vp, vp, i32, i64, vp]),
        'hg_bgu_normal_workspace_bytes': (sz, [i32, i32, i32]),
        'hg_bgu_normal': (ci, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
        'hg_bgu_slice': (ci, [vp, i32, i32, i32, vp, i64, i64, i64, vp, i32, i32, i32, vp]),
        'hg_srgb_to_lab': (ci, [vp, i64, i64, i64, i64, vp, i32, i32, i32, vp]),
        'hg_lab_to_srgb': (ci, [vp, i64, i64, i64, i64, vp, i32, i32, i32, vp]),
        'hg_delta_e_workspace_bytes': (sz, [i32, i32, i32]),
        'hg_delta_e': (ci, [vp, i64, i64, i64, i64, vp, i64, i64, i64, i64, vp, i64, i64, i64, i32, vp, vp, vp, i32, i32,
                            i32, vp, sz, vp]),
        'hg_ssim_tile': (ci, []),
        'hg_ssim_finish_threads': (ci, []),
        'hg_ssim_workspace_bytes': (sz, [i32, i32, i32]),
        'hg_ssim_fwd': (ci, [vp, i64, i64, i64, i64, vp, i64, i64, i64, i64, i32, vp, vp, vp, vp, i32, i32, i32, vp, sz,
                             vp]),
        'hg_ssim_bwd': (ci, [vp, i64, i64, i64, i64, vp, i64, i64, i64, i64, i32, vp, vp, vp, i32, i32, i32, vp]),
        'hg_idt_block_pixels': (ci, []),
        'hg_idt_max_bins': (ci, []),
        'hg_idt_group_pixels': (ci, []),
        'hg_idt_target_chunk': (ci, [i32]),
        'hg_idt_blocks': (ci, [i64]),
        'hg_idt_plane_stride': (i64, [i64]),
        'hg_idt_workspace_bytes': (sz, [i64, i64, i32, i32]),
        'hg_idt_clear': (ci, [vp, i64, vp, i64, vp]),
        'hg_idt_range': (ci, [vp, i64, i64, i64, vp, i32, vp, vp, vp]),
        'hg_idt_hist': (ci, [vp, i64, i64, i64, vp, i32, i32, vp, vp, i32, vp]),
        'hg_idt_table': (ci, [vp, vp, vp, i32, vp, vp, i32, vp]),
        'hg_idt_apply': (ci, [vp, i64, vp, vp, i32, vp, vp, f32, vp, vp, i32, vp]),
        'hg_idt_target_tables': (ci, [vp, i64, i64, i64, vp, i32, i32, vp, vp, vp]),
        'hg_idt_run': (ci, [vp, i64, i64, i64, vp, i64, i64, i64, vp, i32, i32, f32, vp, i32, vp, sz, vp]),
        'hg_palette_max_k': (ci, []),
        'hg_palette_blocks': (ci, [i64]),
        'hg_palette_point_stride': (i64, [i64]),
        'hg_palette_workspace_bytes': (sz, [i32, i64, i32]),
        'hg_palette_quantize': (ci, [vp, i64, i64, i64, i64, vp, i64, i64, i64, vp, i32, i32, i32, vp]),
        'hg_palette_bins': (ci, [vp, i32, i64, vp, i32, vp]),
        'hg_palette_seeds': (ci, [vp, i32, i32, vp, vp]),
        'hg_palette_step': (ci, [vp, vp, i32, i64, vp, i32, vp, vp, i32, vp]),
        'hg_palette_update': (ci, [vp, i32, i32, vp, i32, vp]),
        'hg_palette_run': (ci, [vp, i64, i64, i64, i64, vp, i64, i64, i64, vp, i64, i64, i64, i64, i32, i32, i32, i32, i32, i32,
                                vp, vp, vp, vp, vp, sz, vp]),
        'hg_palette_transfer': (ci, [vp, i64, i64, i64, vp, vp, vp, i32, f32, vp, vp, i32, vp]),
        # include/hg_lut.h
        'hg_lut_max_n': (ci, []),
        'hg_lut_max_pixels': (i64, []),
        'hg_lut_apply_tile': (ci, []),
        'hg_lut_apply_lds_n': (ci, []),
        'hg_lut_splat_lds_n': (ci, []),
        'hg_lut_solve_lds_n': (ci, []),
        'hg_lut_apply_blocks': (ci, [i64]),
        'hg_lut_splat_blocks': (ci, [i64]),
        'hg_lut_workspace_bytes': (sz, [i32]),
        'hg_lut_apply': (ci, [vp, i32, i64, i64, i64, vp, i32, i32, vp, i32, i32, vp]),
        'hg_lut_splat': (ci, [vp, i64, i64, vp, i64, i64, vp, i64, i32, vp, i32, vp]),
        'hg_lut_solve': (ci, [vp, i32, f64, i32, vp, vp, sz, vp]),
        'hg_lut_fit': (ci, [vp, i64, i64, vp, i64, i64, vp, i64, i32, f64, i32, vp, vp, sz, vp]),
        'hg_lut_grad_lds_n': (ci, []),
        'hg_lut_grad_max_pixels': (i64, []),
        'hg_lut_grad_blocks': (ci, [i64]),
        'hg_lut_grad_workspace_bytes': (sz, [i32]),
        'hg_lut_apply_bwd': (ci, [vp, i32, i64, i64, i64, vp, i32, i32, vp, vp, vp, vp, sz, i32, vp]),
        'hg_lut_adam_step': (ci, [vp, vp, vp, vp, vp, i32, f64, f64, f64, f64, f64, i32, vp]),
        # include/hg_regrain.h
        'hg_regrain_tile_h': (ci, []),
        'hg_regrain_tile_w': (ci, []),
        'hg_regrain_max_fused': (ci, []),
        'hg_regrain_plan_fused': (ci, [i32, i32, i32]),
        'hg_regrain_sweep_launches': (ci, [i32, i32]),
        'hg_regrain_levels': (ci, [i32, i32, i32, i32]),
        'hg_regrain_check': (ci, [i32, i32, i32, f64, i32]),
        'hg_regrain_workspace_bytes': (sz, [i32, i32, i32]),
        'hg_regrain_begin': (ci, [vp, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp]),
        'hg_regrain_coef': (ci, [vp, i32, i32, i32, f64, vp, vp, vp]),
        'hg_regrain_sweep': (ci, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        'hg_regrain_finish': (ci, [vp, vp, i32, i32, vp, i32, vp]),
        # include/hg_data.h
        'hg_data_max_ksize': (ci, []),
        'hg_data_item_bytes': (ci, []),
        'hg_data_resample_axis': (ci, [vp, i32, i32, i64, vp, vp, i32, i32, vp]),
        'hg_data_finish': (ci, [vp, i32, i32, vp, vp]),
    }


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} not found: the gfx950 HIP library has not been built. '
            f'Run `python -m histogan_amd.build` (needs hipcc). There is no CPU/PyTorch fallback.')
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


_SIGNATURES = _signatures()
lib = _load()
EXPORTS = tuple(_SIGNATURES)


class HgError(RuntimeError):
    pass


def hist_route(p, weight_grad=False):
    """hg_rgbuv_hist_route for the HgHistParams `p`: the filled HgHistRoute (host only, no launch)."""
    r = HgHistRoute(struct_size=ctypes.sizeof(HgHistRoute))
    check(lib.hg_rgbuv_hist_route(ctypes.byref(p), int(weight_grad), ctypes.byref(r)), 'hg_rgbuv_hist_route')
    return r


def conv_route(B, K, N, Hi, Wi, ksize, stride=1, dgrad=False, fe=False, workspace_bytes=None):
    """hg_conv2d_route: the filled HgConvRoute (host only, no launch).  workspace_bytes None: as the workspace query plans
    (a workspace of any size); 0: no workspace."""
    unlimited = ctypes.c_size_t(-1).value
    q = HgConvQuery(ctypes.sizeof(HgConvQuery), int(dgrad), B, K, N, Hi, Wi, ksize, stride, int(fe),
                    int(workspace_bytes is None or workspace_bytes > 0), unlimited if workspace_bytes is None else workspace_bytes)
    r = HgConvRoute(struct_size=ctypes.sizeof(HgConvRoute))
    check(lib.hg_conv2d_route(ctypes.byref(q), ctypes.byref(r)), 'hg_conv2d_route')
    return r


def _wino_query(B, K, N, H, W, fe, workspace_bytes):
    unlimited = ctypes.c_size_t(-1).value
    return HgWinoQuery(ctypes.sizeof(HgWinoQuery), B, K, N, H, W, int(fe), int(workspace_bytes is None or workspace_bytes > 0),
                       unlimited if workspace_bytes is None else workspace_bytes)


def wino_route(B, K, N, H, W, fe=False, workspace_bytes=None):
    """hg_wino_route: the filled HgWinoRoute of a hg_wino_conv2d call (host only, no launch).  workspace_bytes None: as the
    workspace query plans (a workspace of any size); 0: no workspace."""
    q = _wino_query(B, K, N, H, W, fe, workspace_bytes)
    r = HgWinoRoute(struct_size=ctypes.sizeof(HgWinoRoute))
    check(lib.hg_wino_route(ctypes.byref(q), ctypes.byref(r)), 'hg_wino_route')
    return r


def wino_wgrad_route(B, K, N, H, W, workspace_bytes=None):
    """hg_wino_wgrad_route: the filled HgWinoWgradRoute of a hg_wino_wgrad call (host only, no launch)."""
    q = _wino_query(B, K, N, H, W, False, workspace_bytes)
    r = HgWinoWgradRoute(struct_size=ctypes.sizeof(HgWinoWgradRoute))
    check(lib.hg_wino_wgrad_route(ctypes.byref(q), ctypes.byref(r)), 'hg_wino_wgrad_route')
    return r


def check(rc, what):
    if rc != 0:
        msg = lib.hg_error_string(rc).decode()
        # the two argument errors of the reference are bare Exceptions with these messages
        # (histogram_classes/RGBuvHistBlock.py:90-93, 141-144)
        raise HgError(f'{what}: {msg} (code {rc})')


# ---- cheap host-side plumbing (the train step makes ~1 500 C-ABI calls; each microsecond here is 1.5 ms per step) ------
class NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = NullCtx()


def on_device(device):
    """`with torch.cuda.device(device)` only when `device` is not already current (the context manager costs two driver
    calls; one process drives one GPU, so this is almost always the no-op)."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NULL
    return torch.cuda.device(device)


def raw_stream(device):
    """The caller's current HIP stream on `device` as the void* the C ABI takes."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def stream_of(t):
    """raw_stream of the tensor's device."""
    return raw_stream(t.device)


def f32c(t):
    """`t` as the kernels read it: detached, float32, contiguous (the same storage when it already is both)."""
    t = t.detach()
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def need_gpu(t, what, found='tensor on {}'):
    """Raise unless `t` is a tensor on the GPU.  found: the module's wording of what it got instead ({}: the device)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f'{what}: {found.format(getattr(t, "device", None))}; the MI355X-native path has no CPU implementation')


def workspace(nbytes, device):
    """Scratch of `nbytes` (what a *_workspace_bytes call returned), never empty: the launchers refuse a NULL workspace."""
    return torch.empty(max(nbytes, 4), dtype=torch.uint8, device=device)
