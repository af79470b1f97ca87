// api_core.hip -- the C ABI of include/moptix.h on HIP (gfx950): context, scene staging and upload, LBVH build, accumulation buffer,
// timers, debug read-backs.  The options are in api_options.hip, the launches in api_render.hip, the AOVs in api_aov.hip, the denoiser in api_denoise.hip, the
// collectives in api_comm.hip.  There is no CPU path: every entry point that computes needs a HIP device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_context.h"
#include "pt_lanestack.h"
#include "pt_upload.h"
#include "querykernel.h"

using namespace pt;
using namespace pt::api;

namespace {
std::string g_lastError;   // errors without a context (create)
}

namespace pt { namespace api {

int fail(moptix_context c, int code, const std::string& msg) {
  if (c) c->err = msg; else g_lastError = msg;
  return code;
}
int hipFail(moptix_context c, hipError_t e, const char* what) {
  return fail(c, MOPTIX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

float* accum_ptr(moptix_context c) { return c->accumBound ? c->accumBound : c->dAccum.p; }

int ensure_accum(moptix_context c) {
  const size_t px = (size_t)c->params.width * c->params.height;
  if (c->accumBound) { c->accumPixels = px; return MOPTIX_OK; }
  if (c->dAccum.p && c->accumPixels == px) return MOPTIX_OK;
  // createBuffer(RT_BUFFER_INPUT_OUTPUT, FLOAT3, W, H) zeroed by the host (MinimalOptiX.cpp:144-147)
  HIPCHK(c, c->dAccum.ensure(3 * px), "alloc accuBuffer");
  HIPCHK(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(float) * 3 * px, c->stream), "clear accuBuffer");
  c->accumPixels = px;
  return MOPTIX_OK;
}

int begin_call(moptix_context c, bool withAccum) {
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  const int rc = moptix_sync(c);      // one batch in flight at a time: it finishes (and is timed) first
  return rc != MOPTIX_OK || !withAccum ? rc : ensure_accum(c);
}

int read_back(moptix_context c, std::initializer_list<ReadBack> copies, const char* what) {
  for (const ReadBack& r : copies)
    if (r.dst) HIPCHK(c, hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, c->stream), what);
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

void fill_view(moptix_context c, SceneView& v) {
  memset(&v, 0, sizeof(v));
  const moptix_params& p = c->params;
  v.width = (int)p.width; v.height = (int)p.height;
  v.maxDepth = (int)p.rayMaxDepth; v.minIntensity = p.rayMinIntensity; v.epsT = p.rayEpsilonT;
  v.bg = to_v3(p.bgColor); v.cam = make_cam(p.cam);
  v.nSpheres = (int)c->spheres.size(); v.spheres = c->dSpheres.p; v.sphereMat = c->dSphereMat.p;
  v.nQuads = (int)c->quads.size(); v.quads = c->dQuads.p;
  v.nLights = (int)c->lights.size(); v.lights = c->dLights.p;
  v.nMaterials = (int)c->mats.size(); v.mats = c->dMats.p;
  v.anyDisneyAnalytic = 0;
  for (size_t i = 0; i < c->spheres.size(); i++) if (c->mats[c->sphereMat[i]].kind == MAT_DISNEY) v.anyDisneyAnalytic = 1;
  for (size_t i = 0; i < c->quads.size(); i++) if (c->mats[c->quads[i].mat].kind == MAT_DISNEY) v.anyDisneyAnalytic = 1;
  v.shadowNearest = 0;
  if (c->opt.shadowRule != 0)          // option "shadow_rule": 0 keeps SURVEY A2's order-independent rule whatever the scene holds
    for (const DevMaterial& m : c->mats) if (m.kind == MAT_DISNEY && m.brdfType == BRDF_GLASS) v.shadowNearest = 1;
  v.nTris = c->bvh.nTris; v.rootRef = c->bvh.nTris > 0 ? c->bvh.rootRef : kEmptyRef;
  v.nodes = c->bvh.nodes; v.nodes64 = c->nodeFormatUsed == 64 ? c->bvh.nodes64 : nullptr; v.tris = c->bvh.tris; v.triShade = c->bvh.shade;
  v.triUV = (c->anyUV && c->bvh.nTris > 0) ? c->dFaceUV.p : nullptr;
  v.nTextures = (int)c->textures.size(); v.textures = c->dTextures.p;
}

// Conservative on purpose: a material in the table counts whether or not a primitive uses it.
int scene_features(moptix_context c) {
  int f = c->spheres.empty() ? 0 : FEAT_SPHERES;
  for (const DevMaterial& m : c->mats) {
    if (m.albedoTex != 0) f |= FEAT_TEXTURE;
    if (m.kind == MAT_LAMBERTIAN || m.kind == MAT_METAL || m.kind == MAT_GLASS) f |= FEAT_PLAIN_MATERIALS;
  }
  for (const DevLight& l : c->lights) if (l.shape == LIGHT_SPHERE) f |= FEAT_SPHERE_LIGHT;
  return f;
}

int fill_query_view(moptix_context c, SceneView& v) {
  fill_view(c, v);
  const bool node64 = c->bvh.nodes64 != nullptr && c->opt.nodeFormat != 128 && v.rootRef != kEmptyRef;
  v.nodes64 = node64 ? c->bvh.nodes64 : nullptr;
  return querykernel_blocks(c->numCUs, c->opt.queryBlocksPerCU);
}

int check_ready(moptix_context c) {
  if (!c) return fail(nullptr, MOPTIX_ERR_INVALID, "null context");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "moptix_set_params has not been called");
  if (!c->accelBuilt) return fail(c, MOPTIX_ERR_STATE, "moptix_build_accel has not been called since the scene changed");
  if (c->refit.facesDirty)
    return fail(c, MOPTIX_ERR_STATE, "mesh faces were updated since the tree was fitted: call moptix_refit_accel (keeps the topology) or moptix_build_accel (rebuilds)");
  return MOPTIX_OK;
}

}}  // namespace pt::api

extern "C" {

const char* moptix_version(void) { return "minimaloptix_amd 0.1 (gfx950)"; }

const char* moptix_last_error(moptix_context ctx) { return ctx ? ctx->err.c_str() : g_lastError.c_str(); }

int moptix_create(moptix_context* out, int device) {
  if (!out) return fail(nullptr, MOPTIX_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, MOPTIX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= n) return fail(nullptr, MOPTIX_ERR_INVALID, "device index out of range");
  e = hipSetDevice(device);
  if (e != hipSuccess) return hipFail(nullptr, e, "hipSetDevice");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return hipFail(nullptr, e, "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, MOPTIX_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  moptix_context c = new moptix_context_t();
  c->device = device; c->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { delete c; return hipFail(nullptr, e, "hipStreamCreate"); }
  c->ownStream = true;
  if ((e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess || (e = hipEventCreate(&c->ev2)) != hipSuccess) {
    (void)moptix_destroy(c);                       // releases the stream and whichever events exist
    return hipFail(nullptr, e, "hipEventCreate");
  }
  *out = c;
  return MOPTIX_OK;
}

int moptix_destroy(moptix_context c) {
  if (!c) return MOPTIX_ERR_INVALID;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->release_scene(); c->release_render();
  c->dAccum.release(); c->dRgb8.release();
  c->aov.release(); c->dn.release(); c->tp.release(); c->ad.release(); c->query.release(); c->radiance.release(); c->point.release(); c->box.release(); c->sweep.release(); c->segment.release(); c->obb.release(); c->frustum.release(); c->tri.release(); c->winding.release(); c->refit.drop();
  c->sign.release();
  comm_release(c);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return MOPTIX_OK;
}

int moptix_set_stream(moptix_context c, void* hipStream) {
  if (!c) return MOPTIX_ERR_INVALID;
  (void)hipStreamSynchronize(c->stream);
  if (c->ownStream && c->stream) (void)hipStreamDestroy(c->stream);
  if (hipStream) { c->stream = (hipStream_t)hipStream; c->ownStream = false; }
  else { HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate"); c->ownStream = true; }
  return MOPTIX_OK;
}

int moptix_set_params(moptix_context c, const moptix_params* p) {
  if (!c || !p) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (p->width == 0 || p->height == 0) return fail(c, MOPTIX_ERR_INVALID, "zero-sized launch");
  // the node step sorts entry distances by their bit patterns (pt_path.h ChildKey): distances are clamped to tmin, which must not be negative
  if (!(p->rayEpsilonT >= 0.0f)) return fail(c, MOPTIX_ERR_INVALID, "rayEpsilonT must be >= 0");
  const bool resized = !c->haveParams || p->width != c->params.width || p->height != c->params.height;
  // The node format is chosen by walking the scene's own paths from the camera of the first render after a build
  // (choose_node_format: a device allocation, two probe launches and a stream synchronisation).  A new frame size asks again; a
  // new CAMERA alone does not: a moving camera (updateVideo, MinimalOptiX.cpp:761-778) would otherwise pay that blocking probe in
  // every frame, inside moptix_render_async as well.  set_option("node_format", 0) asks again explicitly.
  if (!c->haveParams || resized) c->formatDecided = false;
  c->params = *p; c->haveParams = true;
  if (resized && !c->accumBound) { c->accumPixels = 0; c->accumPlain = false; }      // reallocated and zeroed at the next use
  if (resized) c->ad.release();                                // the adaptive state describes the old frame's accumulation buffer
  if (resized) c->aov.frame_resized();
  if (resized) c->dn.release();                                // the denoiser's scratch and output are reallocated at its next call
  if (resized) c->tp.release();                                // and the temporal history with them
  return MOPTIX_OK;
}

int moptix_clear_scene(moptix_context c) {
  if (!c) return MOPTIX_ERR_INVALID;
  c->mats.clear(); c->spheres.clear(); c->sphereMat.clear(); c->quads.clear(); c->lights.clear();
  c->facePos.clear(); c->faceNrm.clear(); c->faceHasNrm.clear(); c->faceMat.clear();
  c->faceUV.clear(); c->anyUV = false; c->textures.clear();
  c->sceneDirty = true; c->accelBuilt = false;
  c->tp.drop();                                                // the temporal history belongs to the scene that made it
  c->tp.faces.changed = true;
  if ((c->query.overflow.p || c->radiance.overflow.p || c->point.overflow.p || c->box.overflow.p || c->sweep.overflow.p || c->segment.overflow.p || c->obb.overflow.p || c->frustum.overflow.p || c->tri.overflow.p || c->refit.planned || c->tp.faces.prev.p) && !c->poisoned) {      // a query in flight still uses what is dropped here
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->query.drop(); c->radiance.drop(); c->point.drop(); c->box.drop(); c->sweep.drop(); c->segment.drop(); c->obb.drop(); c->frustum.drop(); c->tri.drop();
    c->tp.faces.release();                                     // the face snapshot too
  }
  c->refit.drop(); c->refit.facesDirty = false; c->refit.hostStale = false; c->refit.facesOnDevice = 0;      // the faces are gone, and the plan with their tree
  sign_release(c);                                             // and the signed queries' topology of them
  winding_release(c);                                          // and the winding queries' table of their tree
  return MOPTIX_OK;
}

int moptix_add_texture(moptix_context c, const float* rgba, int32_t width, int32_t height, int32_t* outTexId) {
  if (!c || !rgba || width <= 0 || height <= 0) return fail(c, MOPTIX_ERR_INVALID, "bad texture");
  moptix_context_t::HostTexture t;
  t.width = width; t.height = height;
  t.rgba.assign(rgba, rgba + 4 * (size_t)width * (size_t)height);
  c->textures.push_back(std::move(t));
  if (outTexId) *outTexId = (int32_t)c->textures.size();     // ids start at 1; 0 is RT_TEXTURE_ID_NULL
  c->sceneDirty = true; c->accelBuilt = false;
  return MOPTIX_OK;
}

int moptix_add_material(moptix_context c, const moptix_material* m, int32_t* outMatId) {
  if (!c || !m) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (m->kind < MOPTIX_MAT_LAMBERTIAN || m->kind > MOPTIX_MAT_LIGHT) return fail(c, MOPTIX_ERR_INVALID, "unknown material kind");
  if (m->kind == MOPTIX_MAT_DISNEY && (m->disney.albedoID < 0 || (size_t)m->disney.albedoID > c->textures.size()))
    return fail(c, MOPTIX_ERR_INVALID, "albedoID names no texture (add textures before the materials that use them)");
  c->mats.push_back(make_dev_material(*m));
  if (outMatId) *outMatId = (int32_t)c->mats.size() - 1;
  c->sceneDirty = true; c->accelBuilt = false;
  return MOPTIX_OK;
}

static int check_mat(moptix_context c, int32_t id) {
  if (id < 0 || id >= (int32_t)c->mats.size()) return fail(c, MOPTIX_ERR_INVALID, "material id out of range");
  return MOPTIX_OK;
}

int moptix_add_spheres(moptix_context c, const moptix_sphere_params* s, const int32_t* matIds, int32_t n) {
  if (!c || n < 0 || (n > 0 && (!s || !matIds))) return fail(c, MOPTIX_ERR_INVALID, "bad argument");
  for (int32_t i = 0; i < n; i++) {
    if (check_mat(c, matIds[i]) != MOPTIX_OK) return MOPTIX_ERR_INVALID;
    c->spheres.push_back(make_dev_sphere(s[i])); c->sphereMat.push_back(matIds[i]);
  }
  c->sceneDirty = true; c->accelBuilt = false;
  return MOPTIX_OK;
}

int moptix_add_quads(moptix_context c, const moptix_quad_params* q, const int32_t* matIds, int32_t n) {
  if (!c || n < 0 || (n > 0 && (!q || !matIds))) return fail(c, MOPTIX_ERR_INVALID, "bad argument");
  for (int32_t i = 0; i < n; i++) {
    if (check_mat(c, matIds[i]) != MOPTIX_OK) return MOPTIX_ERR_INVALID;
    c->quads.push_back(make_dev_quad(q[i], matIds[i]));
  }
  c->sceneDirty = true; c->accelBuilt = false;
  return MOPTIX_OK;
}

int moptix_add_mesh(moptix_context c, const float* positions, int32_t nVerts, const float* normals, int32_t nNormals,
                    const float* texcoords, int32_t nTexcoords, const int32_t* vIdx, const int32_t* nIdx, const int32_t* tIdx,
                    int32_t nFaces, int32_t matId) {
  if (!c || nFaces < 0 || nVerts < 0 || (nFaces > 0 && (!positions || !vIdx))) return fail(c, MOPTIX_ERR_INVALID, "bad argument");
  if (check_mat(c, matId) != MOPTIX_OK) return MOPTIX_ERR_INVALID;
  for (int32_t f = 0; f < 3 * nFaces; f++)
    if (vIdx[f] < 0 || vIdx[f] >= nVerts) return fail(c, MOPTIX_ERR_INVALID, "vertex index out of range");
  const bool meshHasNormals = normals && nNormals > 0 && nIdx;      // normalBuffer.size() != 0, Geometry.cu:136
  const bool meshHasUVs = texcoords && nTexcoords > 0 && tIdx;      // texcoordBuffer.size() != 0, Geometry.cu:141
  for (int32_t f = 0; f < nFaces; f++) {
    bool hasN = meshHasNormals;
    for (int k = 0; k < 3; k++) {
      const float* p = positions + 3 * (size_t)vIdx[3 * f + k];
      c->facePos.push_back(p[0]); c->facePos.push_back(p[1]); c->facePos.push_back(p[2]);
      if (hasN && (nIdx[3 * f + k] < 0 || nIdx[3 * f + k] >= nNormals)) hasN = false;
    }
    for (int k = 0; k < 3; k++) {
      if (hasN) { const float* q = normals + 3 * (size_t)nIdx[3 * f + k]; c->faceNrm.push_back(q[0]); c->faceNrm.push_back(q[1]); c->faceNrm.push_back(q[2]); }
      else { c->faceNrm.push_back(0.f); c->faceNrm.push_back(0.f); c->faceNrm.push_back(0.f); }
    }
    c->faceHasNrm.push_back(hasN ? 1 : 0);
    c->faceMat.push_back(matId);
    TriUV uv; memset(&uv, 0, sizeof(uv));
    if (meshHasUVs) {
      const int32_t* ti = tIdx + 3 * (size_t)f;
      if (ti[0] >= 0 && ti[0] < nTexcoords && ti[1] >= 0 && ti[1] < nTexcoords && ti[2] >= 0 && ti[2] < nTexcoords) {
        uv.u0 = texcoords[2 * (size_t)ti[0]]; uv.v0 = texcoords[2 * (size_t)ti[0] + 1];
        uv.u1 = texcoords[2 * (size_t)ti[1]]; uv.v1 = texcoords[2 * (size_t)ti[1] + 1];
        uv.u2 = texcoords[2 * (size_t)ti[2]]; uv.v2 = texcoords[2 * (size_t)ti[2] + 1];
        uv.hasUV = 1; c->anyUV = true;
      }
    }
    c->faceUV.push_back(uv);
  }
  c->sceneDirty = true; c->accelBuilt = false;
  if (nFaces > 0) sign_release(c);                             // the signed queries' topology describes the faces there were
  return MOPTIX_OK;
}

int moptix_set_lights(moptix_context c, const moptix_light_params* lights, int32_t n) {
  if (!c || n < 0 || (n > 0 && !lights)) return fail(c, MOPTIX_ERR_INVALID, "bad argument");
  c->lights.clear();
  for (int32_t i = 0; i < n; i++) {
    if (lights[i].shape != MOPTIX_LIGHT_SPHERE && lights[i].shape != MOPTIX_LIGHT_QUAD) return fail(c, MOPTIX_ERR_INVALID, "No shape for light.");
    c->lights.push_back(make_dev_light(lights[i]));
  }
  c->sceneDirty = true; c->accelBuilt = false;
  return MOPTIX_OK;
}

int moptix_update_spheres(moptix_context c, int32_t first, const moptix_sphere_params* s, int32_t n) {
  if (!c || !s || first < 0 || n < 0 || (size_t)first + (size_t)n > c->spheres.size()) return fail(c, MOPTIX_ERR_INVALID, "bad sphere range");
  for (int32_t i = 0; i < n; i++) c->spheres[first + i] = make_dev_sphere(s[i]);
  if (c->accelBuilt && n > 0) {
    HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
    HIPCHK(c, hipMemcpyAsync(c->dSpheres.p + first, c->spheres.data() + first, sizeof(DevSphere) * n, hipMemcpyHostToDevice, c->stream), "update spheres");
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  }
  return MOPTIX_OK;
}

int moptix_build_accel(moptix_context c, const char* kind) {
  if (!c || !kind) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  const bool trbvh = !strcmp(kind, "Trbvh") || !strcmp(kind, "Lbvh");
  if (!trbvh && strcmp(kind, "NoAccel")) return fail(c, MOPTIX_ERR_INVALID, std::string("unknown acceleration: ") + kind);
  const int nFaces = (int)c->faceMat.size();
  if (!trbvh && nFaces > 0) return fail(c, MOPTIX_ERR_INVALID, "NoAccel with triangle meshes is not supported; use Trbvh");
  // Whatever happens below, the tree the context holds is not valid for the scene any more: a failed build must not leave accelBuilt set
  // with a freed or stale tree behind it.
  c->accelBuilt = false;
  // The kernels address every scene table with a 32-bit byte offset from its base (pt_types.h at32) and a leaf reference holds its first
  // record in 28 bits; the builder indexes triangles with 32-bit ints.  Checked on the INPUT, before anything is uploaded or built: the node
  // table has at most one four-wide node per two triangles (pt_lbvh.h), so the triangle count bounds every table.
  if ((unsigned long long)nFaces >= (1ull << 28) || (unsigned long long)nFaces * sizeof(Node128) / 2 >= (1ull << 32))
    return fail(c, MOPTIX_ERR_LIMIT, "acceleration structure too large: triangle / node tables must stay below 4 GB (2^28 triangles at most)");
  if ((unsigned long long)c->mats.size() * sizeof(DevMaterial) >= (1ull << 32)) return fail(c, MOPTIX_ERR_LIMIT, "material table must stay below 4 GB");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if (c->refit.hostStale) {                       // moptix_update_faces_device left the newest positions on the device only
    const int rc = fetch_faces(c);
    if (rc != MOPTIX_OK) return rc;
  }
  c->refit.drop();                                // the plan describes the tree that is about to go
  winding_release(c);                             // and so do the winding queries' moments and overflow area
  if ((c->query.overflow.p || c->radiance.overflow.p || c->point.overflow.p || c->box.overflow.p || c->sweep.overflow.p || c->segment.overflow.p || c->obb.overflow.p || c->frustum.overflow.p || c->tri.overflow.p) && !c->poisoned) {      // an asynchronous query in flight still walks the old tree; the area was sized for its depth
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync before the build");
    c->query.drop(); c->radiance.drop(); c->point.drop(); c->box.drop(); c->sweep.drop(); c->segment.drop(); c->obb.drop(); c->frustum.drop(); c->tri.drop();
  }
  HIPCHK(c, c->dMats.upload(c->mats, c->stream), "upload materials");
  HIPCHK(c, c->dSpheres.upload(c->spheres, c->stream), "upload spheres");
  HIPCHK(c, c->dSphereMat.upload(c->sphereMat, c->stream), "upload sphere materials");
  HIPCHK(c, c->dQuads.upload(c->quads, c->stream), "upload quads");
  HIPCHK(c, c->dLights.upload(c->lights, c->stream), "upload lights");
  {  // texture buffers: all texels in one allocation, one descriptor per sampler
    std::vector<float> texels; std::vector<size_t> offs;
    for (const auto& t : c->textures) { offs.push_back(texels.size()); texels.insert(texels.end(), t.rgba.begin(), t.rgba.end()); }
    HIPCHK(c, c->dTexels.upload(texels, c->stream), "upload texels");
    std::vector<DevTexture> desc;
    for (size_t i = 0; i < c->textures.size(); i++)
      desc.push_back(DevTexture{ reinterpret_cast<const v4*>(c->dTexels.p + offs[i]), c->textures[i].width, c->textures[i].height });
    HIPCHK(c, c->dTextures.upload(desc, c->stream), "upload texture descriptors");
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync texture upload");   // staging vectors die here
  }
  lbvh_free(&c->bvh);
  if (nFaces > 0) {
    if (c->anyUV) HIPCHK(c, c->dFaceUV.upload(c->faceUV, c->stream), "upload face texcoords");
    HIPCHK(c, c->dFacePos.upload(c->facePos, c->stream), "upload face positions");
    HIPCHK(c, c->dFaceNrm.upload(c->faceNrm, c->stream), "upload face normals");
    HIPCHK(c, c->dFaceHasNrm.upload(c->faceHasNrm, c->stream), "upload face flags");
    c->refit.facesOnDevice = (size_t)nFaces;
    {
      std::vector<int> words(c->faceMat.size());      // material id + what the face is to a shadow ray (pt_types.h SHADOW_*)
      for (size_t f = 0; f < words.size(); f++) { const DevMaterial& m = c->mats[c->faceMat[f]]; words[f] = face_mat_word(c->faceMat[f], shadow_class(m.kind, m.brdfType)); }
      HIPCHK(c, c->dFaceMat.upload(words, c->stream), "upload face materials");
      HIPCHK(c, hipStreamSynchronize(c->stream), "sync face material upload");      // the staging vector dies here
    }
    size_t glassFaces = 0;
    for (int m : c->faceMat) glassFaces += (c->mats[m].kind == MAT_GLASS || (c->mats[m].kind == MAT_DISNEY && c->mats[m].brdfType == BRDF_GLASS)) ? 1 : 0;
    c->glassFaceShare = (double)glassFaces / (double)nFaces;
    HIPCHK(c, lbvh_build(c->stream, c->dFacePos.p, c->dFaceNrm.p, c->dFaceHasNrm.p, c->dFaceMat.p, nFaces, c->opt.leafSize, c->opt.builder, &c->bvh), "LBVH build");
    // (the same limits again on what was built: belt and braces)
    const unsigned long long lim = 1ull << 32;
    if ((unsigned long long)c->bvh.nTris * sizeof(Tri48) >= lim || (unsigned long long)c->bvh.nTris * sizeof(TriShade) >= lim ||
        (unsigned long long)c->bvh.nNodes * sizeof(Node128) >= lim || (unsigned long long)c->bvh.nTris >= (1ull << 28)) {
      lbvh_free(&c->bvh);
      return fail(c, MOPTIX_ERR_LIMIT, "acceleration structure too large: triangle / node tables must stay below 4 GB (2^28 triangles at most)");
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync after upload");
  c->formatDecided = false;            // choose_node_format at the next render: it needs the camera
  c->sceneDirty = false; c->accelBuilt = true; c->refit.facesDirty = false;
  c->tp.faces.changed = true;   // the device copy of the faces was uploaded afresh (the snapshot stays: the faces keep their upload order)
  c->winding.stale = true;      // the winding queries' moments are computed again for the new tree
  c->sign.stale = true;         // the signed queries' topology stays, their table is computed again from what was uploaded
  c->tiles.forget();            // new scene: forget which tiles had deep paths
  return MOPTIX_OK;
}

int moptix_get_accel_info(moptix_context c, moptix_accel_info* out) {
  if (!c || !out) return MOPTIX_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  out->nTriangles = (uint32_t)c->bvh.nTris; out->nNodes = (uint32_t)c->bvh.nNodes; out->maxLeafSize = (uint32_t)c->bvh.leafSize;
  out->treeDepth = (uint32_t)c->bvh.depth; out->buildMs = c->bvh.buildMs;
  out->nodeBytes = (uint64_t)c->bvh.nNodes * (sizeof(Node128) + (c->bvh.nodes64 ? sizeof(Node64) : 0)); out->triBytes = (uint64_t)c->bvh.nTris * sizeof(Tri48);
  return MOPTIX_OK;
}

int moptix_validate(moptix_context c) {
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (c->mats.empty()) return fail(c, MOPTIX_ERR_STATE, "scene has no materials");
  if (c->spheres.empty() && c->quads.empty() && c->faceMat.empty()) return fail(c, MOPTIX_ERR_STATE, "scene has no geometry");
  for (const DevMaterial& m : c->mats)
    if (m.kind == MAT_DISNEY && m.brdfType != BRDF_NORMAL && m.brdfType != BRDF_GLASS) return fail(c, MOPTIX_ERR_INVALID, "bad brdfType");
  return MOPTIX_OK;
}

int moptix_set_partition(moptix_context c, int32_t rank, int32_t nRanks) {
  if (!c || nRanks < 1 || rank < 0 || rank >= nRanks) return fail(c, MOPTIX_ERR_INVALID, "bad partition");
  if (rank != c->rank || nRanks != c->nRanks) c->tiles.forget();   // other tiles: the deep-path history does not apply
  c->rank = rank; c->nRanks = nRanks;
  return MOPTIX_OK;
}

int moptix_accum_read(moptix_context c, float* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc = ensure_accum(c);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(dstHost, accum_ptr(c), sizeof(float) * 3 * c->accumPixels, hipMemcpyDeviceToHost, c->stream), "read accuBuffer");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_accum_clear(moptix_context c) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc = ensure_accum(c);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipMemsetAsync(accum_ptr(c), 0, sizeof(float) * 3 * c->accumPixels, c->stream), "clear accuBuffer");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  c->accumPlain = false; c->ad.drop();                         // per-pixel counts of a buffer that is gone: zeroed at the next adaptive call
  return MOPTIX_OK;
}

int moptix_accum_device_ptr(moptix_context c, void** devPtr) {
  if (!c || !devPtr) return MOPTIX_ERR_INVALID;
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc = ensure_accum(c);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  *devPtr = accum_ptr(c);
  return MOPTIX_OK;
}

int moptix_accum_bind(moptix_context c, void* devPtr) {
  if (!c) return MOPTIX_ERR_INVALID;
  c->accumBound = (float*)devPtr;
  c->accumPixels = 0;
  c->accumPlain = false; c->ad.drop();                         // another buffer: the adaptive state does not describe it
  return MOPTIX_OK;
}

int moptix_resolve_rgb8(moptix_context c, float nAccumulation, int clearBuffer, uint8_t* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc = ensure_accum(c);
  if (rc != MOPTIX_OK) return rc;
  const size_t bytes = 3 * c->accumPixels;
  HIPCHK(c, c->dRgb8.ensure(bytes), "alloc rgb8");
  HIPCHK(c, launch_resolve_rgb8(c->stream, accum_ptr(c), (int)c->params.width, (int)c->params.height, nAccumulation, clearBuffer, c->dRgb8.p), "resolve kernel");
  HIPCHK(c, hipMemcpyAsync(dstHost, c->dRgb8.p, bytes, hipMemcpyDeviceToHost, c->stream), "read rgb8");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  if (clearBuffer) { c->accumPlain = false; c->ad.drop(); }
  return MOPTIX_OK;
}

int moptix_kernel_time(moptix_context c, double* totalMs, uint64_t* nLaunches, int reset) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (totalMs) *totalMs = c->kernelMs;
  if (nLaunches) *nLaunches = c->nLaunches;
  if (reset) { c->kernelMs = 0.0; c->reduceMs = 0.0; c->nLaunches = 0; }
  return MOPTIX_OK;
}

int moptix_reduce_time(moptix_context c, double* totalMs) {
  if (!c || !totalMs) return MOPTIX_ERR_INVALID;
  *totalMs = c->reduceMs;
  return MOPTIX_OK;
}

int moptix_debug_read_nodes64(moptix_context c, void* nodes64) {
  if (!c || !nodes64) return MOPTIX_ERR_INVALID;
  if (!c->accelBuilt) return fail(c, MOPTIX_ERR_STATE, "no acceleration structure");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if (c->bvh.nNodes > 0 && !c->bvh.nodes64) return fail(c, MOPTIX_ERR_STATE, "this tree has no 64-byte form (a node is wider than 1e10 units)");
  if (c->bvh.nNodes > 0) HIPCHK(c, hipMemcpy(nodes64, c->bvh.nodes64, sizeof(Node64) * c->bvh.nNodes, hipMemcpyDeviceToHost), "read nodes64");
  return MOPTIX_OK;
}

int moptix_debug_read_accel(moptix_context c, void* nodes, void* tris, int32_t* triPrimIds) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (!c->accelBuilt) return fail(c, MOPTIX_ERR_STATE, "no acceleration structure");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if (nodes && c->bvh.nNodes > 0) HIPCHK(c, hipMemcpy(nodes, c->bvh.nodes, sizeof(Node128) * c->bvh.nNodes, hipMemcpyDeviceToHost), "read nodes");
  if ((tris || triPrimIds) && c->bvh.nTris > 0) {
    std::vector<Tri48> h(c->bvh.nTris);
    HIPCHK(c, hipMemcpy(h.data(), c->bvh.tris, sizeof(Tri48) * c->bvh.nTris, hipMemcpyDeviceToHost), "read tris");
    if (tris) memcpy(tris, h.data(), sizeof(Tri48) * h.size());
    if (triPrimIds) for (size_t i = 0; i < h.size(); i++) triPrimIds[i] = h[i].prim;
  }
  return MOPTIX_OK;
}

int moptix_debug_trace(moptix_context c, const float* rays, int32_t n, float* outT, int32_t* outPrim) {
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (n > 0 && (!rays || !outT || !outPrim))) return fail(c, MOPTIX_ERR_INVALID, "bad argument");
  if (n == 0) return MOPTIX_OK;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  float *dR = nullptr, *dT = nullptr; int* dP = nullptr; int* dOvf = nullptr;
  hipError_t e = hipMalloc((void**)&dR, sizeof(float) * 8 * (size_t)n);
  if (e == hipSuccess) e = hipMalloc((void**)&dT, sizeof(float) * (size_t)n);
  if (e == hipSuccess) e = hipMalloc((void**)&dP, sizeof(int) * (size_t)n);
  const size_t ovf = lane_stack_overflow_entries(((size_t)n + 255) / 256 * 256, c->bvh.stackBound, megakernel_lds_stack_entries());
  if (e == hipSuccess && ovf > 0) e = hipMalloc((void**)&dOvf, sizeof(int) * ovf);
  SceneView v; fill_view(c, v);
  if (e == hipSuccess) e = hipMemcpyAsync(dR, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_debug_trace(c->stream, v, dR, n, dT, dP, dOvf);
  if (e == hipSuccess) e = hipMemcpyAsync(outT, dT, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(outPrim, dP, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (dR) (void)hipFree(dR);
  if (dT) (void)hipFree(dT);
  if (dP) (void)hipFree(dP);
  if (dOvf) (void)hipFree(dOvf);
  if (e != hipSuccess) return hipFail(c, e, "debug trace");
  return MOPTIX_OK;
}

}  // extern "C"
