"""ctypes mirror of include/moptix.h and include/moptix_host.h.

The product's compute lives in minimaloptix_amd/lib/libmoptix.so (HIP, gfx950).  This
module only loads it; if the library is missing or there is no MI355X, calls fail loudly
(MoptixError) -- there is no Python/CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
REPO_ROOT = os.path.dirname(_HERE)

MOPTIX_OK = 0
MOPTIX_ERR_INVALID, MOPTIX_ERR_NO_DEVICE, MOPTIX_ERR_HIP, MOPTIX_ERR_STATE, MOPTIX_ERR_LIMIT, MOPTIX_ERR_COMM = -1, -2, -3, -4, -5, -6
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_LIMIT, ERR_COMM = -1, -2, -3, -4, -5, -6
MAT_LAMBERTIAN, MAT_METAL, MAT_GLASS, MAT_DISNEY, MAT_LIGHT = range(5)
BRDF_NORMAL, BRDF_GLASS = 0, 1
LIGHT_SPHERE, LIGHT_QUAD = 0, 1


class MoptixError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("moptix error %d: %s" % (code, msg))
        self.code = code


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tolist(self):
        return [self.x, self.y, self.z]


class Float4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class CamParams(C.Structure):
    _fields_ = [("origin", Float3), ("horizontal", Float3), ("vertical", Float3),
                ("scrLowerLeftCorner", Float3), ("u", Float3), ("v", Float3), ("lensRadius", C.c_float)]


class SphereParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("center", Float3), ("velocity", Float3)]


class QuadParams(C.Structure):
    _fields_ = [("plane", Float4), ("v1", Float3), ("v2", Float3), ("anchor", Float3)]


class DisneyParams(C.Structure):
    _fields_ = [("albedoID", C.c_int32), ("color", Float3), ("emission", Float3),
                ("metallic", C.c_float), ("subsurface", C.c_float), ("specular", C.c_float),
                ("roughness", C.c_float), ("specularTint", C.c_float), ("anisotropic", C.c_float),
                ("sheen", C.c_float), ("sheenTint", C.c_float), ("clearcoat", C.c_float),
                ("clearcoatGloss", C.c_float), ("brdfType", C.c_int32)]


class LightParams(C.Structure):
    _fields_ = [("position", Float3), ("normal", Float3), ("emission", Float3), ("u", Float3), ("v", Float3),
                ("area", C.c_float), ("radius", C.c_float), ("shape", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("albedo", Float3), ("fuzz", C.c_float), ("refIdx", C.c_float),
                ("emission", Float3), ("disney", DisneyParams)]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rayMaxDepth", C.c_uint32),
                ("rayMinIntensity", C.c_float), ("rayEpsilonT", C.c_float), ("bgColor", Float3), ("cam", CamParams)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in
                ("samples", "primaryRays", "bounceRays", "shadowRays", "nodeFetches", "triTests", "closestHits",
                 "lightLoads", "analyticTests", "traversalSteps", "activeLaneSteps", "shadeBatches", "shadeBatchLanes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    @property
    def rays(self):
        return int(self.primaryRays + self.bounceRays + self.shadowRays)


class AccelInfo(C.Structure):
    _fields_ = [("nTriangles", C.c_uint32), ("nNodes", C.c_uint32), ("maxLeafSize", C.c_uint32),
                ("treeDepth", C.c_uint32), ("buildMs", C.c_float), ("nodeBytes", C.c_uint64), ("triBytes", C.c_uint64)]


class SceneSizes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nMaterials", "nSpheres", "nQuads", "nLights", "nVerts", "nNormals",
                                          "nTexcoords", "nFaces", "nMeshes", "nWarnings", "nTextures")]


class RenderResult(C.Structure):
    _fields_ = [("renderMs", C.c_double), ("bvhBuildMs", C.c_float), ("nVertices", C.c_uint64),
                ("nFaces", C.c_uint64), ("nNodes", C.c_uint32), ("treeDepth", C.c_uint32)]


class AovBuffers(C.Structure):
    """moptix_aov_buffers: host (moptix_aov_read) or device (moptix_aov_bind) pointers; NULL members are skipped / keep the own buffer."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("hits", C.c_void_p),
                ("primId", C.c_void_p), ("matId", C.c_void_p)]


class DenoiseParams(C.Structure):
    """moptix_denoise_params (include/moptix.h "denoiser")."""
    _fields_ = [("iterations", C.c_int32), ("normalPower", C.c_int32), ("demodulate", C.c_int32),
                ("sigmaLuminance", C.c_float), ("sigmaDepth", C.c_float)]


class TemporalParams(C.Structure):
    """moptix_temporal_params (include/moptix.h "denoiser: temporal accumulation")."""
    _fields_ = [("alpha", C.c_float), ("alphaMoments", C.c_float), ("depthTolerance", C.c_float), ("normalThreshold", C.c_float),
                ("maxHistory", C.c_int32), ("varianceFrames", C.c_int32)]


class TemporalStats(C.Structure):
    """moptix_temporal_stats: what moptix_temporal_info reports."""
    _fields_ = [("frames", C.c_uint64), ("geometryPixels", C.c_uint64), ("historyPixels", C.c_uint64), ("disoccludedPixels", C.c_uint64),
                ("meanHistory", C.c_float)]


class TemporalFaceStats(C.Structure):
    """moptix_temporal_face_stats: what moptix_temporal_face_info reports."""
    _fields_ = [("trackedFaces", C.c_uint64), ("movedFaces", C.c_uint64), ("movedPixels", C.c_uint64)]


class TemporalBuffers(C.Structure):
    """moptix_temporal_buffers: host pointers for moptix_temporal_read; NULL members are skipped."""
    _fields_ = [("motion", C.c_void_p), ("history", C.c_void_p)]


class AdaptiveParams(C.Structure):
    """moptix_adaptive_params (include/moptix.h "adaptive sampling")."""
    _fields_ = [("threshold", C.c_float), ("minSamples", C.c_int32), ("batch", C.c_int32)]


class AdaptiveStats(C.Structure):
    """moptix_adaptive_stats: what moptix_render_adaptive reports."""
    _fields_ = [("passes", C.c_uint64), ("samplesTraced", C.c_uint64), ("samplesUniform", C.c_uint64),
                ("activePixelsLast", C.c_uint64), ("convergedPixels", C.c_uint64), ("minCount", C.c_uint32), ("maxCount", C.c_uint32)]

    def as_dict(self):
        return dict(passes=int(self.passes), samples_traced=int(self.samplesTraced), samples_uniform=int(self.samplesUniform),
                    active_pixels_last=int(self.activePixelsLast), converged_pixels=int(self.convergedPixels),
                    min_count=int(self.minCount), max_count=int(self.maxCount))


class AdaptiveBuffers(C.Structure):
    """moptix_adaptive_buffers: host pointers for moptix_adaptive_read; NULL members are skipped."""
    _fields_ = [("count", C.c_void_p), ("moments", C.c_void_p), ("error", C.c_void_p), ("converged", C.c_void_p)]


class Hit(C.Structure):
    """moptix_hit: the record of a closest-hit ray query (32 bytes)."""
    _fields_ = [("t", C.c_float), ("prim", C.c_int32), ("mat", C.c_int32), ("u", C.c_float), ("v", C.c_float), ("ng", C.c_float * 3)]


QUERY_CLOSEST, QUERY_ANY = 0, 1
MULTI_COUNT_ALL = 1
MULTI_MAX_HITS = 64


class PointHit(C.Structure):
    """moptix_point_hit: the record of a closest-point query (32 bytes)."""
    _fields_ = [("dist", C.c_float), ("prim", C.c_int32), ("mat", C.c_int32), ("u", C.c_float), ("v", C.c_float), ("p", C.c_float * 3)]


class SegmentHit(C.Structure):
    """moptix_segment_hit: the record of a closest segment query (32 bytes)."""
    _fields_ = [("dist", C.c_float), ("prim", C.c_int32), ("mat", C.c_int32), ("s", C.c_float), ("p", C.c_float * 3), ("feature", C.c_int32)]


POINT_CLOSEST, POINT_ANY, POINT_SIGNED = 0, 1, 2
POINT_MULTI_COUNT_ALL = 1
POINT_MULTI_MAX_NEAR = 64
BOX_ANY, BOX_COUNT = 0, 1
SWEEP_CLOSEST, SWEEP_ANY = 0, 1
SEGMENT_CLOSEST, SEGMENT_ANY = 0, 1
RADIANCE_CLAMP = 1


class RefitInfo(C.Structure):
    """moptix_refit_info: what moptix_get_refit_info reports."""
    _fields_ = [("refitMs", C.c_float), ("sahCost", C.c_double), ("sahCostBuilt", C.c_double), ("has64", C.c_uint32)]

    def as_dict(self):
        return dict(refitMs=float(self.refitMs), sahCost=float(self.sahCost), sahCostBuilt=float(self.sahCostBuilt), has64=int(self.has64))


class SignInfo(C.Structure):
    """moptix_sign_info: what moptix_get_sign_info reports of the faces' topology and the sign table."""
    _fields_ = [(n, C.c_uint32) for n in ("weldedVerts", "edges", "boundaryEdges", "nonManifoldEdges", "flippedEdges", "degenerateFaces",
                                          "closed", "tableBuilds")] + [("signedVolume", C.c_double)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_[:-1]}
        d["signedVolume"] = float(self.signedVolume)
        return d


class WindingInfo(C.Structure):
    """moptix_winding_info: what moptix_get_winding_info reports of the winding queries' moments table."""
    _fields_ = [("tableBuilds", C.c_uint32), ("nodes", C.c_uint32), ("tableBytes", C.c_uint64), ("stale", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return dict(tableBuilds=int(self.tableBuilds), nodes=int(self.nodes), tableBytes=int(self.tableBytes), stale=int(self.stale))


# every symbol include/moptix.h declares (tests check that the library exports all of them)
DEVICE_SYMBOLS = [
    "moptix_create", "moptix_destroy", "moptix_last_error", "moptix_version", "moptix_set_stream",
    "moptix_set_params", "moptix_clear_scene", "moptix_add_texture", "moptix_add_material", "moptix_add_spheres", "moptix_add_quads",
    "moptix_add_mesh", "moptix_set_lights", "moptix_update_spheres", "moptix_build_accel", "moptix_get_accel_info",
    "moptix_validate", "moptix_launch", "moptix_render", "moptix_render_async", "moptix_sync",
    "moptix_render_counted", "moptix_set_partition", "moptix_set_option", "moptix_get_option",
    "moptix_accum_read", "moptix_accum_clear", "moptix_accum_device_ptr", "moptix_accum_bind",
    "moptix_resolve_rgb8", "moptix_kernel_time", "moptix_reduce_time", "moptix_debug_read_accel", "moptix_debug_read_nodes64", "moptix_debug_trace",
    "moptix_comm_unique_id", "moptix_comm_init", "moptix_comm_destroy", "moptix_gather_tiles", "moptix_reduce_frame",
    "moptix_packed_tile_floats", "moptix_pack_tiles", "moptix_unpack_tiles",
    "moptix_render_aovs", "moptix_aov_clear", "moptix_aov_samples", "moptix_aov_read", "moptix_aov_bind",
    "moptix_denoise_defaults", "moptix_denoise", "moptix_denoise_read", "moptix_denoise_bind",
    "moptix_temporal_defaults", "moptix_denoise_temporal", "moptix_temporal_reset", "moptix_temporal_info", "moptix_temporal_read",
    "moptix_temporal_face_info",
    "moptix_adaptive_defaults", "moptix_render_adaptive", "moptix_adaptive_clear", "moptix_adaptive_read", "moptix_adaptive_mean",
    "moptix_adaptive_mean_device", "moptix_adaptive_resolve_rgb8",
    "moptix_query_rays_device", "moptix_query_rays", "moptix_query_rays_multi_device", "moptix_query_rays_multi",
    "moptix_query_radiance_device", "moptix_query_radiance",
    "moptix_query_points_device", "moptix_query_points", "moptix_query_points_signed", "moptix_get_sign_info", "moptix_debug_read_sign_table",
    "moptix_query_points_multi_device", "moptix_query_points_multi",
    "moptix_query_boxes_device", "moptix_query_boxes", "moptix_query_boxes_list_device", "moptix_query_boxes_list",
    "moptix_query_sweeps_device", "moptix_query_sweeps",
    "moptix_query_segments_device", "moptix_query_segments",
    "moptix_query_obbs_device", "moptix_query_obbs", "moptix_query_obbs_list_device", "moptix_query_obbs_list",
    "moptix_query_frusta_device", "moptix_query_frusta", "moptix_query_frusta_list_device", "moptix_query_frusta_list",
    "moptix_query_tris_device", "moptix_query_tris", "moptix_query_tris_list_device", "moptix_query_tris_list",
    "moptix_query_winding_device", "moptix_query_winding", "moptix_get_winding_info", "moptix_debug_read_winding_table",
    "moptix_update_faces", "moptix_update_faces_device", "moptix_refit_accel", "moptix_get_refit_info", "moptix_debug_buffer_addresses",
]
HOST_SYMBOLS = [
    "mohost_last_error", "mohost_scene_build", "mohost_scene_free", "mohost_scene_get_sizes",
    "mohost_scene_get_params", "mohost_scene_warning", "mohost_scene_copy", "mohost_scene_upload",
    "mohost_set_quad_params", "mohost_set_cam_params", "mohost_obj_stats", "mohost_render_scene",
    "mohost_animate_spheres", "mohost_video_camera", "mohost_scene_copy_texcoords", "mohost_scene_texture",
    "mohost_read_image", "mohost_render_scene_adaptive",
]

_dev = None
_host = None


def _load(name):
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise MoptixError(ERR_NO_DEVICE, "%s not found -- run `make` (or __graft_entry__.build()); "
                                          "there is no fallback implementation" % path)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def device_lib():
    global _dev
    if _dev is None:
        L = _load(os.environ.get("MOPTIX_DEVICE_LIB", "libmoptix.so"))   # alternate builds for A/B experiments
        vp, i32, f32p, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.moptix_create.argtypes = [C.POINTER(vp), C.c_int]
        L.moptix_destroy.argtypes = [vp]
        L.moptix_last_error.argtypes = [vp]; L.moptix_last_error.restype = C.c_char_p
        L.moptix_version.restype = C.c_char_p
        L.moptix_set_stream.argtypes = [vp, vp]
        L.moptix_set_params.argtypes = [vp, C.POINTER(Params)]
        L.moptix_clear_scene.argtypes = [vp]
        L.moptix_add_material.argtypes = [vp, C.POINTER(Material), i32p]
        L.moptix_add_texture.argtypes = [vp, f32p, i32, i32, i32p]
        L.moptix_add_spheres.argtypes = [vp, C.POINTER(SphereParams), i32p, i32]
        L.moptix_add_quads.argtypes = [vp, C.POINTER(QuadParams), i32p, i32]
        L.moptix_add_mesh.argtypes = [vp, f32p, i32, f32p, i32, f32p, i32, i32p, i32p, i32p, i32, i32]
        L.moptix_set_lights.argtypes = [vp, C.POINTER(LightParams), i32]
        L.moptix_update_spheres.argtypes = [vp, i32, C.POINTER(SphereParams), i32]
        L.moptix_build_accel.argtypes = [vp, C.c_char_p]
        L.moptix_get_accel_info.argtypes = [vp, C.POINTER(AccelInfo)]
        L.moptix_validate.argtypes = [vp]
        L.moptix_launch.argtypes = [vp, i32]
        L.moptix_render.argtypes = [vp, i32p, i32]
        L.moptix_render_async.argtypes = [vp, i32p, i32]
        L.moptix_sync.argtypes = [vp]
        L.moptix_render_counted.argtypes = [vp, i32p, i32, C.POINTER(Stats)]
        L.moptix_set_partition.argtypes = [vp, i32, i32]
        L.moptix_set_option.argtypes = [vp, C.c_char_p, i32]
        L.moptix_get_option.argtypes = [vp, C.c_char_p, i32p]
        L.moptix_accum_read.argtypes = [vp, f32p]
        L.moptix_accum_clear.argtypes = [vp]
        L.moptix_accum_device_ptr.argtypes = [vp, C.POINTER(vp)]
        L.moptix_accum_bind.argtypes = [vp, vp]
        L.moptix_resolve_rgb8.argtypes = [vp, C.c_float, C.c_int, C.POINTER(C.c_uint8)]
        L.moptix_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.moptix_reduce_time.argtypes = [vp, C.POINTER(C.c_double)]
        L.moptix_debug_read_accel.argtypes = [vp, vp, vp, i32p]
        L.moptix_debug_read_nodes64.argtypes = [vp, vp]
        L.moptix_debug_trace.argtypes = [vp, f32p, i32, f32p, i32p]
        u8p = C.POINTER(C.c_uint8)
        L.moptix_comm_unique_id.argtypes = [u8p]
        L.moptix_comm_init.argtypes = [vp, u8p, i32, i32]
        L.moptix_comm_destroy.argtypes = [vp]
        L.moptix_gather_tiles.argtypes = [vp, i32]
        L.moptix_reduce_frame.argtypes = [vp, i32]
        L.moptix_packed_tile_floats.argtypes = [vp, i32, C.POINTER(C.c_uint64)]
        L.moptix_pack_tiles.argtypes = [vp, i32, i32, vp]
        L.moptix_unpack_tiles.argtypes = [vp, i32, i32, vp]
        L.moptix_render_aovs.argtypes = [vp, i32p, i32]
        L.moptix_aov_clear.argtypes = [vp]
        L.moptix_aov_samples.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.moptix_aov_read.argtypes = [vp, C.POINTER(AovBuffers)]
        L.moptix_aov_bind.argtypes = [vp, C.POINTER(AovBuffers)]
        L.moptix_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
        L.moptix_denoise.argtypes = [vp, C.POINTER(DenoiseParams), C.c_float]
        L.moptix_denoise_read.argtypes = [vp, f32p]
        L.moptix_denoise_bind.argtypes = [vp, vp]
        L.moptix_temporal_defaults.argtypes = [C.POINTER(TemporalParams)]
        L.moptix_denoise_temporal.argtypes = [vp, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_float]
        L.moptix_temporal_reset.argtypes = [vp]
        L.moptix_temporal_info.argtypes = [vp, C.POINTER(TemporalStats)]
        L.moptix_temporal_read.argtypes = [vp, C.POINTER(TemporalBuffers)]
        L.moptix_temporal_face_info.argtypes = [vp, C.POINTER(TemporalFaceStats)]
        L.moptix_adaptive_defaults.argtypes = [C.POINTER(AdaptiveParams)]
        L.moptix_render_adaptive.argtypes = [vp, i32p, i32, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveStats)]
        L.moptix_adaptive_clear.argtypes = [vp]
        L.moptix_adaptive_read.argtypes = [vp, C.POINTER(AdaptiveBuffers)]
        L.moptix_adaptive_mean.argtypes = [vp, f32p]
        L.moptix_adaptive_mean_device.argtypes = [vp, vp]
        L.moptix_adaptive_resolve_rgb8.argtypes = [vp, u8p]
        L.moptix_query_rays_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_rays.argtypes = [vp, f32p, C.c_int64, i32, vp]
        L.moptix_query_rays_multi_device.argtypes = [vp, vp, C.c_int64, i32, C.c_uint32, vp, vp]
        L.moptix_query_rays_multi.argtypes = [vp, f32p, C.c_int64, i32, C.c_uint32, vp, i32p]
        u32p = C.POINTER(C.c_uint32)
        L.moptix_query_radiance_device.argtypes = [vp, vp, C.c_int64, i32p, vp, i32, C.c_uint32, C.c_uint32, vp]
        L.moptix_query_radiance.argtypes = [vp, f32p, C.c_int64, i32p, u32p, i32, C.c_uint32, C.c_uint32, f32p]
        L.moptix_query_points_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_points.argtypes = [vp, f32p, C.c_int64, i32, vp]
        L.moptix_query_points_signed.argtypes = [vp, f32p, C.c_int64, vp]
        L.moptix_query_points_multi_device.argtypes = [vp, vp, C.c_int64, i32, C.c_uint32, vp, vp]
        L.moptix_query_points_multi.argtypes = [vp, f32p, C.c_int64, i32, C.c_uint32, vp, i32p]
        i64p = C.POINTER(C.c_int64)
        L.moptix_query_boxes_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_boxes.argtypes = [vp, f32p, C.c_int64, i32, i32p]
        L.moptix_query_boxes_list_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.moptix_query_boxes_list.argtypes = [vp, f32p, C.c_int64, i64p, i32p, i32p]
        L.moptix_query_sweeps_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_sweeps.argtypes = [vp, f32p, C.c_int64, i32, vp]
        L.moptix_query_segments_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_segments.argtypes = [vp, f32p, C.c_int64, i32, vp]
        L.moptix_query_obbs_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_obbs.argtypes = [vp, f32p, C.c_int64, i32, i32p]
        L.moptix_query_obbs_list_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.moptix_query_obbs_list.argtypes = [vp, f32p, C.c_int64, i64p, i32p, i32p]
        L.moptix_query_frusta_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_frusta.argtypes = [vp, f32p, C.c_int64, i32, i32p]
        L.moptix_query_frusta_list_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.moptix_query_frusta_list.argtypes = [vp, f32p, C.c_int64, i64p, i32p, i32p]
        L.moptix_query_tris_device.argtypes = [vp, vp, C.c_int64, i32, vp]
        L.moptix_query_tris.argtypes = [vp, f32p, C.c_int64, i32, i32p]
        L.moptix_query_tris_list_device.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
        L.moptix_query_tris_list.argtypes = [vp, f32p, C.c_int64, i64p, i32p, i32p]
        L.moptix_query_winding_device.argtypes = [vp, vp, C.c_int64, vp]
        L.moptix_query_winding.argtypes = [vp, f32p, C.c_int64, f32p]
        L.moptix_get_winding_info.argtypes = [vp, C.POINTER(WindingInfo)]
        L.moptix_debug_read_winding_table.argtypes = [vp, vp]
        L.moptix_get_sign_info.argtypes = [vp, C.POINTER(SignInfo)]
        L.moptix_debug_read_sign_table.argtypes = [vp, vp]
        L.moptix_update_faces.argtypes = [vp, i32, i32, f32p, f32p]
        L.moptix_update_faces_device.argtypes = [vp, i32, i32, vp, vp]
        L.moptix_refit_accel.argtypes = [vp]
        L.moptix_get_refit_info.argtypes = [vp, C.POINTER(RefitInfo)]
        L.moptix_debug_buffer_addresses.argtypes = [vp, C.POINTER(C.c_uint64)]
        _dev = L
    return _dev


def host_lib():
    global _host
    if _host is None:
        device_lib()
        L = _load("libmoptix_host.so")
        vp, i32, f32p, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.mohost_last_error.restype = C.c_char_p
        L.mohost_scene_build.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, i32, C.c_float, C.c_int, C.POINTER(vp)]
        L.mohost_scene_free.argtypes = [vp]; L.mohost_scene_free.restype = None
        L.mohost_scene_get_sizes.argtypes = [vp, C.POINTER(SceneSizes)]
        L.mohost_scene_get_params.argtypes = [vp, C.POINTER(Params), C.c_float * 3, C.c_float * 3, C.c_char * 16]
        L.mohost_scene_warning.argtypes = [vp, i32]; L.mohost_scene_warning.restype = C.c_char_p
        L.mohost_scene_copy.argtypes = [vp, C.POINTER(Material), C.POINTER(SphereParams), i32p, C.POINTER(QuadParams), i32p,
                                        C.POINTER(LightParams), f32p, f32p, i32p, i32p, i32p]
        L.mohost_scene_upload.argtypes = [vp, vp]
        L.mohost_scene_copy_texcoords.argtypes = [vp, f32p, i32p]
        L.mohost_scene_texture.argtypes = [vp, i32, i32p, i32p, f32p]
        L.mohost_read_image.argtypes = [C.c_char_p, i32p, i32p, C.POINTER(C.c_uint8), C.c_uint64]
        L.mohost_set_quad_params.argtypes = [C.c_float * 3, C.c_float * 3, C.c_float * 3, C.POINTER(QuadParams)]
        L.mohost_set_quad_params.restype = None
        L.mohost_set_cam_params.argtypes = [C.c_float * 3, C.c_float * 3, C.c_float * 3, C.c_float, C.c_float, C.c_float,
                                            C.c_float, C.POINTER(CamParams)]
        L.mohost_set_cam_params.restype = None
        L.mohost_animate_spheres.argtypes = [C.POINTER(SphereParams), i32, C.c_float, C.POINTER(C.c_float)]
        L.mohost_animate_spheres.restype = None
        L.mohost_video_camera.argtypes = [C.c_float, C.c_float, C.POINTER(CamParams)]
        L.mohost_video_camera.restype = None
        L.mohost_obj_stats.argtypes = [C.c_char_p, i32p, i32p, i32p, i32p]
        L.mohost_render_scene.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(RenderResult)]
        L.mohost_render_scene_adaptive.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                   C.POINTER(AdaptiveParams), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32),
                                                   C.POINTER(C.c_float), C.POINTER(AdaptiveStats)]
        _host = L
    return _host
