"""ctypes binding of liboi_hip.so: the C ABI that the public headers under include/ declare.

SIGS is the one binding table, header file name -> {entry: (restype, argtypes)}, in the order the headers were added;
symbols(header) lists a header's entries.  The table is the reviewed statement of the ABI on the Python side (the headers
are not part of the installed package); tests/helpers/cabi.py holds it against the headers prototype by prototype,
argument by argument, and the struct mirrors below field by field.  Every ctypes.Structure of the package stands in this
module, and an entry that takes one binds it as POINTER of the mirror, never as a plain pointer: that is what lets the
helper find it (tests/test_cabi_cpu.py pins both).

The library handle is module-global (never stored on nn.Module instances, so modules stay
deepcopy-able for the EMA copies the reference trainer makes, src/utils/ema.py:11-12).
There is NO fallback: if the HIP library cannot be loaded every op raises."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# OI_LIB: an alternative build of the same library (A/B experiments, tools/dbg/build_variants.sh); default = the in-tree build
LIB_PATH = os.environ.get("OI_LIB") or os.path.join(_HERE, "liboi_hip.so")
_lock = threading.Lock()
_lib = None

OI_PREC_F32, OI_PREC_BF16X3, OI_PREC_BF16, OI_PREC_BF16X6, OI_PREC_F16X3 = 0, 1, 2, 3, 4
OI_MLP_BLOB_READY = 1
TICKET_WORDS = 4097   # OI_TICKET_WORDS (include/oi_hip.h): device words of an arrival-counter buffer
PRECISIONS = {"f32": OI_PREC_F32, "fp32": OI_PREC_F32, "bf16x3": OI_PREC_BF16X3, "bf16": OI_PREC_BF16,
              "bf16x6": OI_PREC_BF16X6, "f16x3": OI_PREC_F16X3}

_vp, _i, _ll, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t
_u, _ull, _d, _str, _P = ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_double, ctypes.c_char_p, ctypes.POINTER


class CompositeParams(ctypes.Structure):
    """Mirror of `oi_composite_params` (include/oi_hip.h)."""
    _fields_ = ([(n, _vp) for n in ("sdf", "grad", "rgb", "dists", "mid_z", "rays_o", "rays_d", "light_dir", "bg",
                                    "variance", "light")] +
                [("cos_anneal_ratio", _f), ("N", _ll), ("T", _i), ("B", _i)] +
                [(n, _vp) for n in ("weights", "cdf", "alpha", "inside_sphere", "pts_norm", "weight_sum", "weight_max",
                                    "color_fine", "image_no_bg", "image", "shading", "normal", "mask", "z_map",
                                    "specular_map", "diffuse_map", "reduce4", "block_partials", "stats16", "stats_ticket")] +
                [("image_planar", _i)])


PREP_MAX_B = 8


class PrepParams(ctypes.Structure):
    """Mirror of `oi_prep_params` (include/oi_hip.h)."""
    _fields_ = ([(n, (_f * 16) * PREP_MAX_B) for n in ("b2w", "w2b", "c2b")] +
                [("offs", (_f * 2) * PREP_MAX_B), ("bg", (_f * 3) * PREP_MAX_B)] +
                [(n, _i) for n in ("B", "R", "S", "NL")] +
                [(n, _vp) for n in ("kinv", "light_direction", "jitter", "style_w", "style_b", "z", "gw", "gb", "bw", "bb",
                                    "pose_out", "rays_o", "rays_d", "near_", "far_", "light_dir", "z_coarse", "pts_coarse",
                                    "w_out", "gamma", "beta")] +
                [("jitter_normal", _i), ("f3_packed", _vp), ("f3_blob", _vp)])


RELIGHT_LIGHT_FLOATS, RELIGHT_MAX_LIGHTS = 16, 256
# include/oi_local_light.h: floats per local light record; the smallest distance its inverse-square law is evaluated at
LOCAL_LIGHT_FLOATS, LOCAL_LIGHT_MIN_DISTANCE = 20, 1e-3


class RelightParams(ctypes.Structure):
    """Mirror of `oi_relight_params` (include/oi_relight.h)."""
    _fields_ = ([(n, _vp) for n in ("weights", "grad", "rgb", "mid_z", "rays_o", "rays_d", "w2b", "lights", "bg")] +
                [("N", _ll), ("T", _i), ("B", _i), ("L", _i)] +
                [(n, _vp) for n in ("image", "image_no_bg", "shading", "diffuse", "specular")])


class CompositeGrads(ctypes.Structure):
    """Mirror of `oi_composite_grads` (include/oi_hip.h)."""
    _fields_ = [(n, _vp) for n in ("g_weights", "g_weight_sum", "g_color_fine", "g_image_no_bg", "g_image", "g_shading",
                                   "g_normal", "g_mask", "g_z_map", "g_specular_map", "g_diffuse_map", "g_reduce4",
                                   "d_sdf", "d_grad", "d_rgb", "d_variance", "d_light", "d_light_dir", "ray_partials")]


# include/oi_mesh_attr.h
MESH_FLAG_NONFINITE, MESH_FLAG_SMALL_GRADIENT, MESH_FLAG_LIMIT = 1, 2, 4
MESH_MAX_REFINE, MESH_RECORD_BYTES = 8, 27

# include/oi_mesh_tex.h
TEX_MIN_TEXEL, TEX_MAX_TEXEL, TEX_MAX_SIZE = 3, 64, 16384

# include/oi_trace.h
TRACE_MISS, TRACE_HIT, TRACE_LIMIT, TRACE_START_INSIDE, TRACE_NONFINITE, TRACE_BACKFACING = 0, 1, 2, 3, 4, 5
TRACE_MARCH, TRACE_REFINE = 16, 17
TRACE_STATUS_NAMES = {TRACE_MISS: "miss", TRACE_HIT: "hit", TRACE_LIMIT: "limit", TRACE_START_INSIDE: "start_inside",
                      TRACE_NONFINITE: "nonfinite", TRACE_BACKFACING: "backfacing"}
TRACE_DEFAULT_TOL, TRACE_DEFAULT_OMEGA, TRACE_DEFAULT_MAX_STEPS, TRACE_DEFAULT_BIAS = 1e-5, 1.0, 64, 1e-2
TRACE_MAX_STEPS, TRACE_COUNT_WORDS = 1024, 1026


class TraceState(ctypes.Structure):
    """Mirror of `oi_trace_state` (include/oi_trace.h)."""
    _fields_ = [("N", _ll)] + [(n, _vp) for n in ("rays_o", "rays_d", "near_", "far_", "t", "status", "steps", "bracket",
                                                  "side", "active", "points", "counts")]


class SurfaceParams(ctypes.Structure):
    """Mirror of `oi_surface_params` (include/oi_trace.h)."""
    _fields_ = ([("N", _ll), ("n_hit", _ll), ("L", _i)] +
                [(n, _vp) for n in ("rays_o", "rays_d", "t", "status", "hit_slot", "hit_points", "grad", "rgb", "w2b",
                                    "lights", "bg", "visibility", "depth", "position", "normal", "normal_world", "albedo",
                                    "mask", "image")])


# include/oi_occlusion.h
OCCLUSION_MAX_SAMPLES = 256


class SurfaceAoParams(ctypes.Structure):
    """Mirror of `oi_surface_ao_params` (include/oi_occlusion.h): SurfaceParams' fields, then the occlusion factor."""
    _fields_ = SurfaceParams._fields_ + [("ambient_occlusion", _vp)]


# include/oi_aa.h
AA_MAX_SAMPLES, AA_DEFAULT_PLANE, AA_DEFAULT_COS = 64, 0.5, 0.5

# include/oi_mesh_band.h
BAND_MIN_RES, BAND_MAX_RES = 2, 1024

# include/oi_trace_batch.h
TRACE_BATCH_MAX_ELEMS = 1024


class TraceBatch(ctypes.Structure):
    """Mirror of `oi_trace_batch` (include/oi_trace_batch.h)."""
    _fields_ = [("s", TraceState), ("E", _i), ("live", _vp)]


# include/oi_envlight.h
ENV_COEFFS, ENV_FLOATS, ENV_MAX_ENVS = 9, 27, 256


class EnvShadeParams(ctypes.Structure):
    """Mirror of `oi_env_shade_params` (include/oi_envlight.h)."""
    _fields_ = ([("N", _ll), ("n_hit", _ll), ("F", _i)] +
                [(n, _vp) for n in ("status", "hit_slot", "rgb", "transfer", "envs", "bg", "shading", "image")])


# include/oi_envbounce.h
BOUNCE_FLOATS = 27


class EnvShadeBounceParams(ctypes.Structure):
    """Mirror of `oi_env_shade_bounce_params` (include/oi_envbounce.h): EnvShadeParams' fields, then the bounce transfer and
    its output."""
    _fields_ = EnvShadeParams._fields_ + [("bounce", _vp), ("indirect", _vp)]


# include/oi_envgloss.h
ENVGLOSS_MIN_SHININESS, ENVGLOSS_MAX_SHININESS, ENVGLOSS_CHUNK = 1, 4096, 2048

# include/oi_scene.h
SCENE_MAX_RESOLUTION = 32768


class SceneShadeParams(ctypes.Structure):
    """Mirror of `oi_scene_shade_params` (include/oi_scene.h)."""
    _fields_ = ([(n, _i) for n in ("E", "W", "S", "L")] + [("n_pad", _ll)] +
                [(n, _vp) for n in ("owner", "owner_ray", "rays_o", "rays_d", "t", "vis_slot", "hit_points", "grad", "rgb", "w2b",
                                    "b2w", "lights", "bg", "visibility", "depth", "position", "normal", "normal_world", "albedo",
                                    "mask", "instance", "image")])


# include/oi_scene_light.h
class SceneShadeAoParams(ctypes.Structure):
    """Mirror of `oi_scene_shade_ao_params` (include/oi_scene_light.h): the scene's shade parameters, then the occlusion
    factor."""
    _fields_ = [("s", SceneShadeParams), ("ambient_occlusion", _vp)]


class SceneOcclusionParams(ctypes.Structure):
    """Mirror of `oi_scene_occlusion_params` (include/oi_scene_light.h)."""
    _fields_ = ([(n, _i) for n in ("L", "S", "j0", "Sc", "ambient")] +
                [("seed", _u), ("bias", _f), ("distance", _f), ("n_pad", _ll), ("n_vis", _ll)] +
                [(n, _vp) for n in ("hit_points", "grad", "offset", "elem", "pixel", "position", "normal", "lights", "radius", "w2b")])


# include/oi_ground.h
GROUND_FLOATS = 12
GROUND_RAYS_CAP, GROUND_RAYS_HEMISPHERE, GROUND_RAYS_LOCAL = 0, 1, 2

# include/oi_occlusion_batch.h
OCCLUSION_BATCH_SHADOW, OCCLUSION_BATCH_CAP, OCCLUSION_BATCH_HEMISPHERE, OCCLUSION_BATCH_LOCAL = 0, 1, 2, 3

# include/oi_raster.h
RASTER_MAX_VIEWS, RASTER_MAX_RESOLUTION, RASTER_MAX_COORD = 1024, 16384, 1 << 22
RASTER_DROPPED, RASTER_EMPTY, RASTER_SMALL, RASTER_LARGE = 0, 1, 2, 3
RASTER_VERTEX, RASTER_TEXTURE = 0, 1


SIGS = {
    # include/oi_hip.h: the drop-in boundary, what replaces the reference's modules
    "oi_hip.h": {
        "oi_version": (_i, []),
        "oi_arch": (_str, []),
        "oi_last_error": (_str, []),
        "oi_film_params": (_i, [_vp] * 10 + [_i, _i, _vp]),
        "oi_film_params_bwd": (_i, [_vp] * 16 + [_i, _i, _vp]),
        "oi_mlp_packed_bytes": (_sz, [_i]),
        "oi_mlp_pack_weights": (_i, [_vp] * 11 + [_i, _vp]),
        "oi_mlp_pack_status": (_i, [_vp, _vp]),
        "oi_mlp_scratch_bytes": (_sz, [_i, _ll]),
        "oi_mlp_scratch_bytes_prec": (_sz, [_i, _ll, _i]),
        "oi_sdf_mlp_fwd": (_i, [_vp] * 9 + [_i, _ll, _i, _i, _vp]),
        "oi_sdf_mlp_fwd_ex": (_i, [_vp] * 9 + [_i, _ll, _i, _i, _i, _vp]),
        "oi_mlp_f3_blob_offset": (_sz, [_i, _ll]),
        "oi_mlp_f3_blob_bytes": (_sz, []),
        "oi_selftest_sincos": (_i, [_vp, _vp, _vp, _ll, _i, _vp]),
        "oi_selftest_q24": (_i, [_vp, _vp, _ll, _i, _vp]),
        "oi_selftest_cu_slots": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
        "oi_mlp_bwd_scratch_bytes": (_sz, [_i, _ll]),
        "oi_mlp_bwd_scratch_bytes_capped": (_sz, [_i, _ll, _sz]),
        "oi_mlp_bwd_small_floats": (_i, []),
        "oi_sdf_mlp_bwd": (_i, [_vp] * 15 + [_sz, _i, _ll, _i, _i, _vp]),
        "oi_sdf_mlp_bwd_feat": (_i, [_vp] * 16 + [_sz, _i, _ll, _i, _i, _vp]),
        "oi_color_head_fwd": (_i, [_vp] * 4 + [_ll] + [_vp] * 5 + [_i, _ll, _vp]),
        "oi_color_head_bwd_workspace_bytes": (_sz, [_i, _ll]),
        "oi_color_head_bwd": (_i, [_vp] * 4 + [_ll] + [_vp] * 9 + [_ll] + [_vp] * 5 + [_sz, _i, _ll, _vp]),
        "oi_composite_bwd": (_i, [_P(CompositeParams), _P(CompositeGrads), _vp]),
        "oi_render_stats": (_i, [_vp, _i, _ll, _i, _vp, _vp]),
        "oi_composite_num_blocks": (_i, [_ll]),
        "oi_gen_rays": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
        "oi_gen_rays_light": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "oi_coarse_samples": (_i, [_vp] * 5 + [_ll, _i, _vp, _vp, _vp]),
        "oi_prep_render": (_i, [_P(PrepParams), _vp]),
        "oi_upsample": (_i, [_vp] * 4 + [_ll, _i, _i, _f, _vp, _vp, _vp, _vp]),
        "oi_upsample_mid": (_i, [_vp] * 4 + [_ll, _i, _i, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
        "oi_merge_sorted": (_i, [_vp] * 4 + [_ll, _i, _i, _vp, _vp, _vp]),
        "oi_midpoints": (_i, [_vp] * 3 + [_ll, _i, _f, _vp, _vp, _vp, _vp]),
        "oi_composite_fwd": (_i, [_P(CompositeParams), _vp]),
        "oi_conv4x4_fwd": (_i, [_vp] * 4 + [_i] * 7 + [_f, _vp]),
        "oi_conv4x4_fwd_into": (_i, [_vp] * 4 + [_i] * 7 + [_f, _f, _i, _vp]),
        "oi_conv4x4_fwd_arena": (_i, [_vp] * 4 + [_i] * 7 + [_f, _f, _i, _ll, _vp]),
        "oi_conv4x4_dgrad": (_i, [_vp] * 3 + [_i] * 7 + [_vp]),
        "oi_conv4x4_wgrad": (_i, [_vp] * 3 + [_i] * 7 + [_vp]),
        "oi_conv4x4_dgrad_masked": (_i, [_vp, _vp, _f, _vp, _vp] + [_i] * 7 + [_vp]),
        "oi_conv4x4_wgrad_masked": (_i, [_vp, _vp, _f, _vp, _vp] + [_i] * 8 + [_vp]),
        "oi_conv4x4_bwd_masked": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _vp] + [_i] * 8 + [_vp]),
        "oi_conv4x4_bwd_pre": (_i, [_vp, _vp, _f, _vp, _vp, _f, _vp, _vp] + [_i] * 8 + [_vp]),
        "oi_conv4x4_dgrad_pre": (_i, [_vp, _vp, _vp, _f, _vp] + [_i] * 7 + [_vp]),
        "oi_lrelu_mask_mul": (_i, [_vp] * 3 + [_ll, _f, _vp]),
        "oi_channel_sum": (_i, [_vp, _vp, _i, _i, _i, _vp]),
        "oi_upfirdn2d": (_i, [_vp] * 3 + [_i] * 14 + [_f, _vp]),
        "oi_ada_geom_fwd": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
        "oi_ada_geom_sep_supported": (_i, [_i] * 3),
        "oi_ada_geom_sep_fwd": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
        "oi_ada_geom_sep_adj": (_i, [_vp] * 5 + [_i] * 8 + [_vp]),
        "oi_ada_pad_up2": (_i, [_vp] * 3 + [_i] * 8 + [_vp]),
        "oi_disc_fwd_small_workspace_floats": (_sz, [_i] * 6),
        "oi_disc_fwd_small": (_i, [_vp] * 4 + [_i] * 4 + [_vp] * 9 + [_i] * 6 + [_f, _vp]),
        "oi_disc_large_packed_bytes": (_sz, [_vp, _i, _i]),
        "oi_disc_large_pack": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
        "oi_disc_large_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
        "oi_disc_fwd_large": (_i, [_vp] * 5 + [_sz, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
        "oi_disc_graph_create": (_i, [_vp, _i, _vp] + [_i] * 4 + [_vp] * 9 + [_i] * 6 + [_f]),
        "oi_disc_graph_launch": (_i, [_vp, _vp, _vp, _vp]),
        "oi_disc_fwd_small128_workspace_floats": (_sz, [_i] * 6),
        "oi_disc_fwd_small128": (_i, [_vp] * 4 + [_i] * 4 + [_vp] * 10 + [_i] * 4 + [_f, _vp]),
        "oi_disc_graph_create128": (_i, [_vp, _i, _vp] + [_i] * 4 + [_vp] * 10 + [_i] * 4 + [_f]),
        "oi_disc_graph_launch_eager": (_i, [_vp, _vp, _vp, _vp, _vp]),
        "oi_ada_theta_xint_scale": (_i, [_ull] + [_i] * 7 + [_f] * 4 + [_vp, _vp]),
        "oi_disc_graph_launch_ada": (_i, [_vp, _vp, _ull, _f, _f, _f, _f, _vp, _i, _vp]),
        "oi_disc_graph_destroy": (None, [_vp]),
        "oi_outputs_prezeroed_stream": (_i, [_vp, _i]),
        "oi_light_dir_fwd": (_i, [_vp, _vp, _vp, _i, _vp]),
        "oi_light_dir_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
        "oi_gan_losses_fwd": (_i, [_vp] * 5 + [_f, _vp, _i, _i, _ll, _vp]),
        "oi_gan_losses_bwd": (_i, [_vp] * 6 + [_f, _vp, _vp, _vp, _i, _i, _ll, _vp]),
        "oi_stage_inputs": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
        "oi_render_scalars_fwd": (_i, [_vp, _f, _vp, _vp]),
        "oi_zero_fill": (_i, [_vp, _ll, _vp]),
        "oi_scalar_glue": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "oi_render_scalars_bwd": (_i, [_vp, _vp, _vp, _f, _vp, _vp]),
        "oi_weighted_sum_fwd": (_i, [_vp, _vp, _i, _vp, _vp]),
        "oi_weighted_sum_bwd": (_i, [_vp, _vp, _i, _vp, _vp]),
        "oi_affine_grid_sample_fwd": (_i, [_vp] * 3 + [_i] * 6 + [_vp]),
        "oi_affine_grid_sample_bwd": (_i, [_vp] * 3 + [_i] * 6 + [_vp]),
        "oi_fused_bias_act": (_i, [_vp] * 4 + [_i, _i, _f, _f, _ll, _ll, _i, _vp]),
        "oi_grid_sample_fwd": (_i, [_vp] * 3 + [_i] * 6 + [_vp]),
        "oi_grid_sample_bwd": (_i, [_vp] * 5 + [_i] * 6 + [_vp]),
        "oi_reflect_pad_fwd": (_i, [_vp, _vp] + [_i] * 7 + [_vp]),
        "oi_reflect_pad_bwd": (_i, [_vp, _vp] + [_i] * 7 + [_vp]),
        "oi_mt_chunk_elems": (_i, []),
        "oi_multi_adam": (_i, [_vp, _i, _f, _f, _f, _f, _f, _f, _f, _f, _vp]),
        "oi_multi_rmsprop": (_i, [_vp, _i, _f, _f, _f, _f, _vp]),
        "oi_multi_lerp": (_i, [_vp, _i, _f, _vp]),
        "oi_multi_copy": (_i, [_vp, _i, _vp]),
        # mesh extraction: the reference's extract_fields point source (renderer.py:15-31) and mcubes.marching_cubes (:33-41)
        "oi_sdf_lattice": (_i, [_vp] * 3 + [_i] + [_vp] * 3 + [_i] * 3 + [_f, _vp, _i, _i, _vp]),
        "oi_mc_workspace_bytes": (_sz, [_i] * 3),
        "oi_mc_count": (_i, [_vp] + [_i] * 3 + [_f, _vp, _sz, _P(_ll), _vp]),
        "oi_mc_emit": (_i, [_vp] + [_i] * 3 + [_f, _vp, _sz, _vp, _ll, _vp, _ll, _vp]),
    },
    # include/oi_relight.h: relighting of a captured render (no reference counterpart, so not in oi_hip.h)
    "oi_relight.h": {
        "oi_relight_fwd": (_i, [_P(RelightParams), _vp]),
    },
    # include/oi_mesh_attr.h: the vertex pass of the intrinsic mesh export (no reference counterpart either)
    "oi_mesh_attr.h": {
        "oi_mesh_vertex_world": (_i, [_vp, _ll] + [_vp] * 3 + [_i] * 3 + [_vp, _vp, _vp]),
        "oi_mesh_newton": (_i, [_vp] * 4 + [_ll] + [_f] * 4 + [_vp, _vp, _vp]),
        "oi_mesh_attr_finalize": (_i, [_vp] * 4 + [_ll, _f] + [_vp] * 5),
        "oi_mesh_vertex_record": (_i, [_vp] * 3 + [_ll, _vp, _vp]),
    },
    # include/oi_trace.h: sphere-traced surface rendering (no reference counterpart either)
    "oi_trace.h": {
        "oi_trace_begin": (_i, [_P(TraceState), _vp]),
        "oi_trace_step": (_i, [_P(TraceState), _vp, _ll, _i, _f, _f, _vp]),
        "oi_trace_finish": (_i, [_P(TraceState), _vp, _vp, _vp, _vp]),
        "oi_trace_shadow_begin": (_i, [_P(TraceState), _vp, _vp, _ll, _vp, _i, _vp, _f, _vp]),
        "oi_trace_visibility": (_i, [_vp, _vp, _ll, _ll, _i, _vp, _vp]),
        "oi_surface_shade": (_i, [_P(SurfaceParams), _vp]),
    },
    # include/oi_occlusion.h: soft shadows and ambient occlusion on the traced surface (an addition to oi_trace.h; its
    # entries work on an oi_trace_state)
    "oi_occlusion.h": {
        "oi_occlusion_light_begin": (_i, [_P(TraceState), _vp, _vp, _vp, _ll, _vp, _vp, _i, _i, _vp, _f, _u, _vp]),
        "oi_occlusion_ambient_begin": (_i, [_P(TraceState), _vp, _vp, _vp, _ll, _i, _f, _f, _u, _vp]),
        "oi_occlusion_step": (_i, [_P(TraceState), _vp, _ll, _i, _f, _f, _vp]),
        "oi_occlusion_resolve": (_i, [_vp, _vp, _ll, _ll, _i, _i, _vp, _vp]),
        "oi_surface_shade_ao": (_i, [_P(SurfaceAoParams), _vp]),
    },
    # include/oi_mesh_band.h: narrow-band mesh extraction (accelerates renderer.py:15-41; no reference counterpart either)
    "oi_mesh_band.h": {
        "oi_band_workspace_bytes": (_sz, [_i] * 4),
        "oi_band_classify": (_i, [_vp] + [_i] * 5 + [_d] * 3 + [_f, _f, _d, _vp, _vp, _sz, _P(_ll), _P(_f), _vp]),
        "oi_sdf_lattice_band": (_i, [_vp] * 3 + [_i] + [_vp] * 3 + [_i] * 4 + [_vp, _ll, _f, _vp, _i, _i, _vp]),
    },
    # include/oi_trace_batch.h: E latents / views in one chain of trace steps (an addition to oi_trace.h)
    "oi_trace_batch.h": {
        "oi_sdf_mlp_fwd_segments": (_i, [_vp] * 5 + [_i, _ll, _ll, _i, _i, _vp]),
        "oi_trace_batch_begin": (_i, [_P(TraceBatch), _vp]),
        "oi_trace_batch_step": (_i, [_P(TraceBatch), _vp, _ll, _i, _f, _f, _vp]),
        "oi_trace_batch_finish": (_i, [_P(TraceBatch), _vp, _vp, _vp]),
        "oi_trace_batch_gather": (_i, [_P(TraceBatch), _vp, _ll, _vp, _vp]),
    },
    # include/oi_envlight.h: SH environment lights and per-pixel transfer on the traced surface (an addition to
    # oi_occlusion.h)
    "oi_envlight.h": {
        "oi_env_project_partial_floats": (_sz, [_i, _i, _i]),
        "oi_env_project": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
        "oi_transfer_resolve": (_i, [_vp, _vp, _vp, _ll, _ll, _i, _vp, _vp, _vp]),
        "oi_transfer_normal": (_i, [_vp, _vp, _ll, _ll, _vp, _vp, _vp]),
        "oi_env_shade": (_i, [_P(EnvShadeParams), _vp]),
    },
    # include/oi_scene.h: many instances in one scene image (an addition to oi_trace_batch.h)
    "oi_scene.h": {
        "oi_scene_begin": (_i, [_P(TraceBatch), _vp, _vp, _vp, _i, _i, _vp]),
        "oi_scene_resolve": (_i, [_P(TraceBatch), _vp, _i, _i, _vp, _vp, _vp]),
        "oi_scene_visible": (_i, [_P(TraceBatch), _vp, _vp, _i, _i, _vp, _vp, _vp]),
        "oi_scene_shade": (_i, [_P(SceneShadeParams), _vp]),
        "oi_scene_points": (_i, [_P(TraceBatch), _vp, _vp, _ll, _vp, _ll] + [_vp] * 6),
        "oi_scene_shadow_begin": (_i, [_P(TraceBatch), _vp, _vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _i, _vp, _f, _vp]),
        "oi_scene_visibility": (_i, [_vp] * 5 + [_i, _ll, _i, _ll, _i, _vp, _vp]),
    },
    # include/oi_envgloss.h: the Phong lobe under an environment map (an addition to oi_envlight.h; no struct of its own)
    "oi_envgloss.h": {
        "oi_env_prefilter_partial_floats": (_sz, [_i] * 5),
        "oi_env_prefilter": (_i, [_vp, _i, _i, _i, _f, _i, _i, _vp, _vp, _vp]),
        "oi_occlusion_lobe_begin": (_i, [_P(TraceState), _vp, _vp, _vp, _vp, _ll, _i, _f, _f, _u, _vp]),
        "oi_env_shade_glossy": (_i, [_P(EnvShadeParams)] + [_vp] * 6 + [_i, _i, _i, _P(_i), _vp, _vp, _vp, _vp]),
    },
    # include/oi_scene_light.h: sampled secondary rays between the instances of a scene (an addition to oi_scene.h,
    # oi_occlusion.h and oi_envlight.h)
    "oi_scene_light.h": {
        "oi_scene_point_pixels": (_i, [_P(TraceBatch), _vp, _vp, _i, _i, _vp, _ll, _vp, _vp]),
        "oi_scene_occlusion_begin": (_i, [_P(TraceBatch), _P(SceneOcclusionParams), _vp]),
        "oi_trace_batch_step_anyhit": (_i, [_P(TraceBatch), _vp, _ll, _i, _f, _f, _vp]),
        "oi_scene_occlusion_resolve": (_i, [_vp] * 5 + [_i, _ll, _i, _i, _i, _i, _ll, _i, _i, _vp, _vp, _vp]),
        "oi_scene_transfer_resolve": (_i, [_vp] * 7 + [_i, _ll, _i, _i, _i, _ll, _i, _i, _vp, _vp]),
        "oi_scene_transfer_normal": (_i, [_vp, _ll] + [_vp] * 4 + [_i, _ll, _i, _vp, _vp]),
        "oi_scene_shade_ao": (_i, [_P(SceneShadeAoParams), _vp]),
    },
    # include/oi_envbounce.h: one diffuse interreflection bounce in the transfer of a captured view (an addition to
    # oi_envlight.h)
    "oi_envbounce.h": {
        "oi_bounce_resolve": (_i, [_vp] * 6 + [_ll, _ll, _ll, _i, _vp, _vp, _vp]),
        "oi_env_shade_bounce": (_i, [_P(EnvShadeBounceParams), _vp]),
    },
    # include/oi_scene_gloss.h: the Phong lobe under an environment map in a scene of many instances (an addition to
    # oi_scene_light.h and oi_envgloss.h; no struct of its own: the lobe's begin takes oi_scene_light.h's parameters)
    "oi_scene_gloss.h": {
        "oi_scene_lobe_begin": (_i, [_P(TraceBatch), _P(SceneOcclusionParams), _vp, _vp, _ll, _f, _vp]),
        "oi_scene_reflect": (_i, [_vp, _vp, _vp, _ll] + [_vp] * 4 + [_i, _ll, _i, _vp, _vp]),
        "oi_env_shade_glossy_dirs": (_i, [_P(EnvShadeParams), _vp, _vp, _vp, _i, _i, _i, _P(_i), _vp, _vp, _vp, _vp]),
    },
    # include/oi_scene_bounce.h: one diffuse interreflection bounce between the instances of a scene (an addition to
    # oi_scene_light.h and oi_envbounce.h; no struct of its own: plain arguments, and the batch of oi_trace_batch.h)
    "oi_scene_bounce.h": {
        "oi_scene_bounce_nearest": (_i, [_vp, _vp, _i, _ll, _vp, _vp]),
        "oi_scene_bounce_visible": (_i, [_P(TraceBatch), _vp, _vp, _vp, _vp]),
        "oi_scene_bounce_resolve": (_i, [_vp] * 5 + [_ll] + [_vp] * 5 + [_i, _ll, _i, _i, _i, _ll, _i, _i, _vp, _vp]),
    },
    # include/oi_local_light.h: point, spot and sphere lights in the world, with shadow rays that end at the light (an
    # addition to oi_occlusion.h and oi_scene_light.h; no struct of its own: their structs with `lights` at local records)
    "oi_local_light.h": {
        "oi_local_light_begin": (_i, [_P(TraceState), _vp, _vp, _vp, _ll, _vp, _i, _i, _vp, _f, _u, _vp]),
        "oi_surface_shade_local": (_i, [_P(SurfaceAoParams), _vp]),
        "oi_scene_local_light_begin": (_i, [_P(TraceBatch), _P(SceneOcclusionParams), _vp]),
        "oi_scene_shade_local": (_i, [_P(SceneShadeAoParams), _vp]),
    },
    # include/oi_mesh_tex.h: the per-triangle texture atlas of the textured mesh export (an addition to oi_mesh_attr.h; no
    # struct of its own: plain arguments)
    "oi_mesh_tex.h": {
        "oi_tex_layout": (_i, [_ll, _i, _P(_i), _P(_i), _P(_i)]),
        "oi_tex_uv": (_i, [_ll, _i, _vp, _vp]),
        "oi_tex_points": (_i, [_vp, _vp, _ll, _ll, _i, _vp, _vp, _vp]),
        "oi_tex_store": (_i, [_vp, _vp, _ll, _ll, _i, _ll] + [_vp] * 5),
    },
    # include/oi_aa.h: adaptive anti-aliasing of the traced surface (an addition to oi_trace.h; no struct of its own: plain
    # arguments, and the state of oi_trace.h)
    "oi_aa.h": {
        "oi_aa_classify": (_i, [_vp] * 4 + [_ll, _i, _i, _f, _f, _vp, _vp, _vp, _vp]),
        "oi_aa_begin": (_i, [_P(TraceState), _vp, _vp, _vp, _i, _vp, _ll, _vp, _i, _vp]),
        "oi_aa_resolve": (_i, [_vp, _vp, _vp, _ll, _ll, _i, _i, _vp, _vp]),
    },
    # include/oi_scene_aa.h: adaptive anti-aliasing of a scene of many instances (an addition to oi_scene.h and oi_aa.h; no
    # struct of its own)
    "oi_scene_aa.h": {
        "oi_scene_aa_classify": (_i, [_vp] * 5 + [_i, _ll, _ll, _i, _f, _f, _vp, _vp, _vp, _vp]),
        "oi_scene_aa_begin": (_i, [_P(TraceBatch), _vp, _vp, _vp, _i, _i, _vp, _ll, _vp, _i, _vp]),
        "oi_aa_resolve_strided": (_i, [_vp, _vp, _ll, _vp, _ll, _ll, _i, _i, _vp, _vp]),
    },
    # include/oi_ground.h: a ground plane that catches the instances' shadows (an addition to oi_scene_light.h and
    # oi_local_light.h; no struct of its own: plain arguments, and the rays' begin takes oi_scene_light.h's parameters)
    "oi_ground.h": {
        "oi_ground_begin": (_i, [_vp, _vp, _i] + [_vp] * 5 + [_i, _i, _vp, _vp, _vp, _vp]),
        "oi_ground_rays_begin": (_i, [_P(TraceBatch), _P(SceneOcclusionParams), _i, _vp, _vp, _i, _vp, _vp, _vp]),
        "oi_ground_resolve": (_i, [_vp, _i, _ll, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
        "oi_ground_shade": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _ll, _vp, _i, _i] + [_vp] * 12),
        "oi_ground_occlude": (_i, [_P(TraceBatch), _vp, _vp, _vp, _ll, _f, _vp]),
    },
    # include/oi_occlusion_batch.h: the secondary rays and the shade of E views in one chain (an addition to oi_trace_batch.h,
    # oi_occlusion.h and oi_local_light.h; no struct of its own: the batch, oi_occlusion.h's shade parameters, plain arguments)
    "oi_occlusion_batch.h": {
        "oi_occlusion_batch_begin": (_i, [_P(TraceBatch), _i] + [_vp] * 4 + [_ll, _ll, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _u, _vp]),
        "oi_occlusion_batch_resolve": (_i, [_vp, _vp, _vp, _i, _ll, _ll, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
        "oi_surface_shade_batch": (_i, [_P(SurfaceAoParams), _i, _ll, _i, _vp]),
    },
    # include/oi_raster.h: the mesh rasteriser, a G-buffer for oi_trace.h's shade from a triangle mesh (an addition to
    # oi_trace.h and oi_mesh_tex.h; no struct of its own: plain arguments)
    "oi_raster.h": {
        "oi_raster_setup": (_i, [_vp] * 3 + [_i, _i, _vp, _vp, _ll, _ll, _f, _ll] + [_vp] * 7),
        "oi_raster_fill": (_i, [_vp] * 3 + [_i, _i, _vp, _vp, _ll, _ll] + [_vp] * 7),
        "oi_raster_resolve": (_i, [_vp] * 3 + [_i, _i, _vp, _vp, _ll, _ll, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 15),
    },
}


class OiHipError(RuntimeError):
    pass


def symbols(header):
    """The entry points that include/<header> declares, sorted."""
    return sorted(SIGS[header])


def load():
    """Load (once) and return the ctypes handle.  Raises OiHipError when the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # PyTorch bundles its own libamdhip64.so.7; liboi_hip.so needs the same SONAME.  Importing torch FIRST makes the
        # dynamic loader resolve our dependency to the runtime torch already mapped -- one HIP runtime per process.
        # (Loaded the other way round, /opt/rocm's copy comes in through our RUNPATH, torch then maps its own by
        # path, and launches on torch's streams fail with "no ROCm-capable device is detected".)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise OiHipError(
                f"{LIB_PATH} not found: build it with `python object-intrinsics_amd/build.py` (hipcc, gfx950). "
                "oi_amd has no CPU or PyTorch fallback for its kernels.")
        lib = ctypes.CDLL(LIB_PATH)
        for entries in SIGS.values():
            for name, (res, args) in entries.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    raise OiHipError(f"{LIB_PATH} does not export {name}; rebuild the library")
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().oi_last_error()
        raise OiHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
