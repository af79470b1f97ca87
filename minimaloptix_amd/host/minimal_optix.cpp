#include "minimal_optix.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <random>
#include <stdexcept>

#include <hip/hip_runtime_api.h>      // hipMalloc / hipFree of the adaptive path's mean buffer: nothing else of HIP is used on the host

#include "../csrc/pt_rng.h"
#include "image_io.h"

using namespace moptix;

MinimalOptiX::MinimalOptiX(int device) {
  int rc = moptix_create(&context, device);
  if (rc != MOPTIX_OK) throw std::runtime_error(std::string("moptix_create: ") + moptix_last_error(nullptr));
  setupContext();
}

MinimalOptiX::~MinimalOptiX() { if (context) moptix_destroy(context); }

void MinimalOptiX::check(int rc, const char* what) {
  if (rc != MOPTIX_OK) throw std::runtime_error(std::string(what) + ": " + moptix_last_error(context));
}

// MinimalOptiX.cpp:130-152.  Ray types, entry points and the OptiX stack size have no
// equivalent (the megakernel is iterative); the context variables travel in moptix_params
// together with the camera and are pushed by setupScene().
void MinimalOptiX::setupContext() {
  canvas.assign((size_t)fixedWidth * fixedHeight * 3, 0);
}

// utils_host.cpp:118-122
int MinimalOptiX::randSeed() {
  if (reproducibleSeeds) return (int)pt::tea16(launchCounter++, baseSeed);
  static auto engine = std::minstd_rand(std::random_device{}());
  static auto randGen = std::uniform_real_distribution<float>(-1.f, 1.f);
  return int(randGen(engine) * (float)std::numeric_limits<int>::max());
}

// MinimalOptiX.cpp:154-357
void MinimalOptiX::setupScene() {
  aabb.invalidate();
  switch (sceneId) {
    case SCENE_SPHERES: buildSpheresScene(scene, fixedWidth, fixedHeight); break;
    case SCENE_COFFEE: setupScene("coffee"); return;
    case SCENE_BEDROOM: setupScene("bedroom"); return;
    case SCENE_DININGROOM: setupScene("diningroom"); return;
    case SCENE_STORMTROOPER: setupScene("stormtrooper"); return;
    case SCENE_SPACESHIP: setupScene("spaceship"); return;
    case SCENE_CORNELL: setupScene("cornell"); return;
    case SCENE_HYPERION: setupScene("hyperion"); return;
    case SCENE_DRAGON: setupScene("dragon"); return;
    case SCENE_SPHERES_VIDEO:                                                                          // :355
      buildRandomSpheresScene(scene, 256, fixedWidth, fixedHeight);
      videoParams.spheresParams = scene.spheres; videoParams.angle = 0.f;
      break;
    case SCENE_CORNELL_QUADS: buildCornellQuadsScene(scene, fixedWidth, fixedHeight); break;
    case SCENE_RANDOM_SPHERES_500: buildRandomSpheresScene(scene, 497, fixedWidth, fixedHeight); break;
    case SCENE_DINING_STANDIN: buildDiningStandInScene(scene, baseSceneFolder, 6, fixedWidth, fixedHeight); break;
    case SCENE_MILLION_STANDIN: buildProceduralMillionScene(scene, 1000000, fixedWidth, fixedHeight); break;
    case SCENE_COFFEE_POT_STANDIN: buildCoffeePotStandInScene(scene, baseSceneFolder, fixedWidth, fixedHeight); break;
  }
  scene.params.rayMaxDepth = rayMaxDepth; scene.params.rayMinIntensity = rayMinIntensity; scene.params.rayEpsilonT = rayEpsilonT;
  aabb = scene.aabb; nVertices = scene.nVertices; nFaces = scene.nFaces;
  check(upload(scene, context), "upload scene");
}

// MinimalOptiX.cpp:359-538 (+ the camera placement of :258-353)
void MinimalOptiX::setupScene(const char* sceneName) {
  buildFileScene(scene, baseSceneFolder, sceneName, fixedWidth, fixedHeight, skipMissingMeshes);
  scene.params.rayMaxDepth = rayMaxDepth; scene.params.rayMinIntensity = rayMinIntensity; scene.params.rayEpsilonT = rayEpsilonT;
  aabb = scene.aabb; nVertices = scene.nVertices; nFaces = scene.nFaces;
  if (verbose) for (const std::string& w : scene.warnings) fprintf(stderr, "[MinimalOptiX] %s\n", w.c_str());
  check(upload(scene, context), "upload scene");
}

// Communicator of this rank: rank 0 makes the id (ncclGetUniqueId behind moptix_comm_unique_id) and publishes it as a file
// (written under a temporary name, then renamed); the other ranks wait for the file.  moptix_comm_init is collective.
void MinimalOptiX::setupCommunicator() {
  if (commIdFile.empty()) throw std::runtime_error("commIdFile is not set (needed for nRanks > 1)");
  uint8_t id[MOPTIX_COMM_ID_BYTES];
  if (rank == 0) {
    check(moptix_comm_unique_id(id), "comm unique id");
    const std::string tmp = commIdFile + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f || fwrite(id, 1, sizeof(id), f) != sizeof(id)) { if (f) fclose(f); throw std::runtime_error("cannot write " + tmp); }
    fclose(f);
    if (rename(tmp.c_str(), commIdFile.c_str()) != 0) throw std::runtime_error("cannot publish " + commIdFile);
  } else {
    bool got = false;
    for (int tries = 0; tries < 1200 && !got; tries++) {         // two minutes
      FILE* f = fopen(commIdFile.c_str(), "rb");
      if (f) { got = fread(id, 1, sizeof(id), f) == sizeof(id); fclose(f); }
      if (!got) std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    if (!got) throw std::runtime_error("no communicator id at " + commIdFile);
  }
  check(moptix_comm_init(context, id, rank, nRanks), "comm init");
}

// MinimalOptiX.cpp:540-560
void MinimalOptiX::renderScene(bool autoSave, std::string fileNamePrefix) {
  if (nRanks < 1 || rank < 0 || rank >= nRanks) throw std::runtime_error("bad rank / nRanks");
  check(moptix_set_partition(context, rank, nRanks), "set partition");
  setupScene();
  check(moptix_validate(context), "validate");                 // :542
  const bool multi = nRanks > 1 || !commIdFile.empty();
  if (adaptive && (multi || autoSave)) throw std::runtime_error("adaptive sampling is for one rank and one image (no tile split, no progressive snapshots)");
  if (multi) { setupCommunicator(); autoSave = false; }         // progressive snapshots would need a gather each: one-GPU only
  moptix_get_accel_info(context, &lastAccel);
  if (canvas.size() != (size_t)fixedWidth * fixedHeight * 3) canvas.assign((size_t)fixedWidth * fixedHeight * 3, 0);
  moptix_kernel_time(context, nullptr, nullptr, 1);
  std::vector<int32_t> seeds(nSuperSampling);
  for (uint i = 0; i < nSuperSampling; ++i) seeds[i] = randSeed();   // :545 one seed per launch
  lastSeeds = seeds;
  if (adaptive) { renderAdaptive(fileNamePrefix); return; }
  uint checkpoint = 1;
  uint done = 0;
  while (done < nSuperSampling) {
    // the reference launches once per sample (:546); the launches between two snapshots are
    // fused into one kernel -- per pixel the samples are still added in launch order.
    uint upto = nSuperSampling;
    if (autoSave) { while (checkpoint <= done) checkpoint *= 2; upto = std::min(checkpoint, nSuperSampling); }
    check(moptix_render(context, seeds.data() + done, (int32_t)(upto - done)), "render");
    done = upto;
    if (autoSave && done == checkpoint) {                       // :547-553
      updateContent((float)done, false);
      saveCurrentFrame(false, fileNamePrefix + "_" + std::to_string(done));
    }
  }
  if (multi) check(moptix_gather_tiles(context, 0), "gather tiles");      // the frame's one exchange: every rank's tiles to rank 0
  if (denoise && rank == 0) saveDenoised(fileNamePrefix);      // before the resolve below clears accuBuffer
  updateContent((float)nSuperSampling, true);                   // :555 (ranks > 0: clears their accuBuffer; their canvas is partial)
  if (autoSave) saveCurrentFrame(false, fileNamePrefix);        // :556-558
  uint64_t n = 0;
  moptix_kernel_time(context, &lastRenderMs, &n, 0);
  if (verbose) fprintf(stderr, "vertices: %zu faces: %zu\n", nVertices, nFaces);   // :559
}

// renderScene()'s launches and resolve when `adaptive` is set
void MinimalOptiX::renderAdaptive(std::string fileNamePrefix) {
  check(moptix_adaptive_clear(context), "adaptive clear");
  check(moptix_render_adaptive(context, lastSeeds.data(), (int32_t)lastSeeds.size(), &adaptiveParams, &lastAdaptive), "adaptive render");
  const size_t px = (size_t)fixedWidth * fixedHeight;
  adaptiveCount.assign(px, 0u); adaptiveError.assign(px, 0.f);
  moptix_adaptive_buffers b = { adaptiveCount.data(), nullptr, adaptiveError.data(), nullptr };
  check(moptix_adaptive_read(context, &b), "read adaptive state");
  check(moptix_adaptive_resolve_rgb8(context, canvas.data()), "adaptive resolve");
  if (denoise) {
    // the per-pixel mean as the accumulator of a denoise call that divides by 1; binding drops the adaptive state, which is read by now
    float* mean = nullptr;
    if (hipMalloc((void**)&mean, sizeof(float) * 3 * px) != hipSuccess) throw std::runtime_error("cannot allocate the mean buffer");
    try {
      check(moptix_adaptive_mean_device(context, mean), "adaptive mean");
      check(moptix_accum_bind(context, mean), "bind mean");
      saveDenoised(fileNamePrefix, false, 1.0f);
      check(moptix_accum_bind(context, nullptr), "unbind mean");
    } catch (...) { moptix_accum_bind(context, nullptr); (void)hipFree(mean); throw; }
    (void)hipFree(mean);
  }
  check(moptix_accum_clear(context), "clear");                  // as updateContent(n, true) leaves it
  uint64_t n = 0;
  moptix_kernel_time(context, &lastRenderMs, &n, 0);
  if (verbose) {
    const moptix_adaptive_stats& s = lastAdaptive;
    fprintf(stderr, "adaptive: threshold %g, %d + n x %d seeds: %llu passes, %llu of %llu samples traced (%.1f %%), %llu pixels active and %llu converged after the last pass, %u to %u samples per pixel\n",
            (double)adaptiveParams.threshold, adaptiveParams.minSamples, adaptiveParams.batch, (unsigned long long)s.passes, (unsigned long long)s.samplesTraced,
            (unsigned long long)s.samplesUniform, s.samplesUniform ? 100.0 * (double)s.samplesTraced / (double)s.samplesUniform : 0.0,
            (unsigned long long)s.activePixelsLast, (unsigned long long)s.convergedPixels, s.minCount, s.maxCount);
    fprintf(stderr, "vertices: %zu faces: %zu\n", nVertices, nFaces);
  }
}

void MinimalOptiX::saveAdaptive(std::string fileNamePrefix) {
  const size_t px = (size_t)fixedWidth * fixedHeight;
  if (adaptiveCount.size() != px || adaptiveError.size() != px) throw std::runtime_error("no adaptive render to save");
  std::vector<float> img(3 * px);
  const std::string base = outputDir + "/" + (fileNamePrefix.empty() ? std::string("frame") : fileNamePrefix);
  for (int which = 0; which < 2; which++) {
    for (size_t i = 0; i < px; i++) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = which == 0 ? (float)adaptiveCount[i] : adaptiveError[i];
    const std::string name = base + (which == 0 ? "_count.pfm" : "_error.pfm");
    if (!writePFM(name, img.data(), fixedWidth, fixedHeight)) throw std::runtime_error("cannot write " + name);
    if (verbose) fprintf(stderr, "Adaptive-sampling image saved to %s\n", name.c_str());
  }
}

// MinimalOptiX.cpp:43-66 (normalise, clamp, flip rows, optionally clear) -- done on the device
void MinimalOptiX::updateContent(float nAccumulation, bool clearBuffer) {
  check(moptix_resolve_rgb8(context, nAccumulation, clearBuffer ? 1 : 0, canvas.data()), "resolve");
}

// MinimalOptiX.cpp:68-84
void MinimalOptiX::saveCurrentFrame(bool popUpDialog, std::string fileNamePrefix) {
  (void)popUpDialog;
  std::string fileName = outputDir + "/" + (fileNamePrefix.empty() ? std::string("frame") : fileNamePrefix) + ".png";
  if (!writePNG(fileName, canvas.data(), fixedWidth, fixedHeight)) throw std::runtime_error("cannot write " + fileName);
  if (verbose) fprintf(stderr, "Image saved to %s\n", fileName.c_str());
}

void MinimalOptiX::saveAovs(std::string fileNamePrefix) {
  check(moptix_aov_clear(context), "AOV clear");
  check(moptix_render_aovs(context, lastSeeds.data(), (int32_t)lastSeeds.size()), "render AOVs");
  const size_t px = (size_t)fixedWidth * fixedHeight;
  std::vector<float> albedo(3 * px), normal(3 * px), depth(px), hits(px), depth3(3 * px);
  moptix_aov_buffers b = { albedo.data(), normal.data(), depth.data(), hits.data(), nullptr, nullptr };
  check(moptix_aov_read(context, &b), "read AOVs");
  uint64_t n = 0;
  check(moptix_aov_samples(context, &n), "AOV samples");
  const float fn = (float)(n > 0 ? n : 1);
  for (size_t i = 0; i < 3 * px; i++) { albedo[i] = albedo[i] / fn; normal[i] = normal[i] / fn; }
  for (size_t i = 0; i < px; i++) depth3[3 * i] = depth3[3 * i + 1] = depth3[3 * i + 2] = hits[i] > 0.f ? depth[i] / hits[i] : 0.f;
  const std::string base = outputDir + "/" + (fileNamePrefix.empty() ? std::string("frame") : fileNamePrefix);
  for (auto& f : { std::make_pair(std::string("_albedo.pfm"), &albedo), std::make_pair(std::string("_normal.pfm"), &normal), std::make_pair(std::string("_depth.pfm"), &depth3) }) {
    if (!writePFM(base + f.first, f.second->data(), fixedWidth, fixedHeight)) throw std::runtime_error("cannot write " + base + f.first);
    if (verbose) fprintf(stderr, "AOV saved to %s\n", (base + f.first).c_str());
  }
}

void MinimalOptiX::saveDenoised(std::string fileNamePrefix, bool temporal, float nAccumulation) {
  if (!(nAccumulation > 0.f)) nAccumulation = (float)nSuperSampling;
  check(moptix_aov_clear(context), "AOV clear");
  check(moptix_render_aovs(context, lastSeeds.data(), (int32_t)lastSeeds.size()), "render AOVs");
  moptix_denoise_params p;
  check(moptix_denoise_defaults(&p), "denoise defaults");
  p.iterations = denoiseIterations;
  if (temporal) {
    moptix_temporal_params t;
    check(moptix_temporal_defaults(&t), "temporal defaults");
    check(moptix_denoise_temporal(context, &p, &t, nAccumulation), "temporal denoise");
  } else {
    check(moptix_denoise(context, &p, nAccumulation), "denoise");
  }
  const size_t px = (size_t)fixedWidth * fixedHeight;
  std::vector<float> out(3 * px);
  check(moptix_denoise_read(context, out.data()), "read denoised");
  std::vector<uint8_t> rgb(3 * px);
  for (size_t i = 0; i < px; i++) {
    const size_t row = i / fixedWidth, col = i % fixedWidth;
    uint8_t* dst = rgb.data() + 3 * ((fixedHeight - 1 - row) * fixedWidth + col);
    for (int c = 0; c < 3; c++) {
      const float v = std::min(std::max(out[3 * i + c], 0.0f), 1.0f);
      dst[c] = (uint8_t)(((uint32_t)(v * 65535.0f + 0.5f)) >> 8);      // as k_resolve_rgb8 (updateContent)
    }
  }
  const std::string base = outputDir + "/" + (fileNamePrefix.empty() ? std::string("frame") : fileNamePrefix) + "_denoised";
  if (!writePFM(base + ".pfm", out.data(), fixedWidth, fixedHeight)) throw std::runtime_error("cannot write " + base + ".pfm");
  if (!writePNG(base + ".png", rgb.data(), fixedWidth, fixedHeight)) throw std::runtime_error("cannot write " + base + ".png");
  if (verbose) fprintf(stderr, "Denoised image saved to %s.pfm / .png\n", base.c_str());
}

// MinimalOptiX.cpp:587-592
void MinimalOptiX::animate(float time) { animateSpheres(videoParams, time); }

// MinimalOptiX.cpp:761-778: advance the physics, rewrite every sphere, new orbit camera, re-render
void MinimalOptiX::updateVideo() {
  animate(0.002f);
  check(moptix_update_spheres(context, 0, videoParams.spheresParams.data(), (int32_t)videoParams.spheresParams.size()), "update spheres");
  videoCamera(videoParams, (float)fixedWidth / (float)fixedHeight, scene.params.cam);
  check(moptix_set_params(context, &scene.params), "set params");
  std::vector<int32_t> seeds(nSuperSampling);
  for (uint i = 0; i < nSuperSampling; ++i) seeds[i] = randSeed();
  check(moptix_render(context, seeds.data(), (int32_t)nSuperSampling), "render");
  if (denoiseTemporal && rank == 0) {                          // before the resolve below clears accuBuffer
    lastSeeds = seeds;
    saveDenoised(videoPrefix + "_video" + std::to_string(videoStep), true);
  }
  videoStep++;
  updateContent((float)nSuperSampling, true);
}

// MinimalOptiX.cpp:594-605 (generateVideo is dead code in the reference; frames are saved as PNG)
void MinimalOptiX::record(int frames, const char* filename, bool saveFrames) {
  (void)filename;
  for (int i = 0; i < frames; ++i) {
    updateVideo();
    if (saveFrames) saveCurrentFrame(false, "video" + std::to_string(i));
  }
}

// MinimalOptiX.cpp:112-117
void MinimalOptiX::videoDemo() {
  nSuperSampling = 128u;
  sceneId = SCENE_SPHERES_VIDEO;
  renderScene(false, "VIDEO");
  record(1000, "test.mp4", true);
}

// MinimalOptiX.cpp:86-110, restricted to the scenes whose assets exist
void MinimalOptiX::imageDemo() {
  nSuperSampling = 4096u;
  sceneId = SCENE_COFFEE;
  renderScene(true, "coffee");
}
