// vb_plugin.hip — device model plugins (VB_TARGET_PLUGIN): the user's log density as a
// gfx950 code object, loaded with the HIP module API and launched on the materialised
// path in place of the host callback (include/viabel_amd.h, "Device model plugins").
//
// What is checked: the image's bytes (vb_plugin_image.hpp) before HIP parses them, the
// launch record again as the device holds it, the handle, its device and the dimension
// at every use.  What is not: the kernel itself.  It runs with the library's pointers; a
// kernel that writes outside logp [n] and grad [n][D] corrupts the process like any other
// out-of-bounds kernel would.
#include "../../include/viabel_amd.h"
#include "vb_internal.hpp"
#include "vb_plugin_image.hpp"

#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <set>
#include <string>

struct vb_plugin {
  vb_ctx* owner = nullptr;     // the context it was loaded on (its stream is synchronised
                               // before the module is unloaded)
  int device = 0;
  hipModule_t module = nullptr;
  hipFunction_t function = nullptr;
  int32_t launch[3] = {0, 0, 0};   // block, rows_per_block, dmax
  int refs = 1;                    // guarded by g_mu
};

namespace {

std::mutex g_mu;
std::set<const vb_plugin*>* g_live = nullptr;   // never freed: handles may outlive statics

bool live_locked(const vb_plugin* p) { return p && g_live && g_live->count(p) != 0; }

#define PL_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (void)hipGetLastError();                                                               \
      return vbk::vb_set_error(VB_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    }                                                                                        \
  } while (0)

}  // namespace

namespace vbk {

int plugin_view(const vb_plugin* p, int device, long long dim, long long n_data, PluginTarget* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!live_locked(p))
    return vb_set_error(VB_EINVAL, "plugin target: vb_target.user is not a live vb_plugin handle");
  if (p->device != device)
    return vb_set_error(VB_EINVAL, "plugin target: the plugin was loaded on GPU %d but the context is "
                        "on GPU %d", p->device, device);
  if (p->launch[2] != 0 && dim > p->launch[2])
    return vb_set_error(VB_EINVAL, "plugin target: dimension %lld is larger than the model's dmax %d",
                        dim, p->launch[2]);
  if (out) *out = PluginTarget{p->function, p->launch[0], p->launch[1], n_data};
  return VB_OK;
}

int plugin_retain(vb_plugin* p) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!live_locked(p)) return vb_set_error(VB_EINVAL, "not a live vb_plugin handle");
  ++p->refs;
  return VB_OK;
}

int plugin_target_eval(const PluginTarget& p, int D, long long n, const double* data,
                       const double* x, double* logp, double* grad, hipStream_t st) {
  if (!p.function) return vb_set_error(VB_EINVAL, "plugin target without a loaded kernel");
  if (n <= 0) return VB_OK;
  const long long blocks = (n + p.rows_per_block - 1) / p.rows_per_block;
  if (blocks > 0x7fffffffLL)
    return vb_set_error(VB_EINVAL, "plugin target: %lld rows need %lld blocks, more than a grid holds", n,
                        blocks);
  long long n_data = data ? p.n_data : 0;
  void* args[] = {&x, &n, &D, &data, &n_data, &logp, &grad};
  PL_HIP(hipModuleLaunchKernel(p.function, (unsigned)blocks, 1, 1, (unsigned)p.block, 1, 1, 0, st, args,
                               nullptr));
  return VB_OK;
}

}  // namespace vbk

extern "C" {

int vb_plugin_check_image(const void* image, int64_t bytes, const char* kernel) {
  char err[400];
  if (!vbimg::check_image(image, bytes, kernel, nullptr, err, sizeof err))
    return vbk::vb_set_error(VB_EINVAL, "%s", err);
  return VB_OK;
}

int vb_plugin_load(vb_ctx* ctx, const void* image, int64_t bytes, const char* kernel,
                   vb_plugin** out) {
  if (!out) return vbk::vb_set_error(VB_EINVAL, "null output pointer");
  *out = nullptr;
  // 1. the bytes, before HIP sees them
  vbimg::Image img;
  char err[400];
  if (!vbimg::check_image(image, bytes, kernel, &img, err, sizeof err))
    return vbk::vb_set_error(VB_EINVAL, "%s", err);
  int device = 0;
  hipStream_t stream = nullptr;
  if (int rc = vbk::ctx_device_stream(ctx, &device, &stream)) return rc;   // selects the device
  // 2. the module (HIP copies what it needs: the caller's bytes are not kept), from the
  // code object itself so a bundle's other entries are never parsed
  hipModule_t mod = nullptr;
  PL_HIP(hipModuleLoadData(&mod, static_cast<const unsigned char*>(image) + img.elf_off));
  auto drop = [&](int rc) {
    (void)hipModuleUnload(mod);
    return rc;
  };
  // 3. the kernel
  hipFunction_t fn = nullptr;
  hipError_t e = hipModuleGetFunction(&fn, mod, kernel);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return drop(vbk::vb_set_error(VB_EINVAL, "plugin: no kernel '%.100s' in the module: %s", kernel,
                                  hipGetErrorString(e)));
  }
  // 4. the launch record as the device holds it
  const std::string rec_name = std::string(kernel) + "_launch";
  hipDeviceptr_t rec_ptr = nullptr;
  size_t rec_bytes = 0;
  e = hipModuleGetGlobal(&rec_ptr, &rec_bytes, mod, rec_name.c_str());
  if (e != hipSuccess || rec_bytes < sizeof(int32_t) * 3) {
    (void)hipGetLastError();
    return drop(vbk::vb_set_error(VB_EINVAL, "plugin: no launch record '%s' of 12 bytes in the module",
                                  rec_name.c_str()));
  }
  int32_t rec[3] = {0, 0, 0};
  e = hipMemcpy(rec, rec_ptr, sizeof rec, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return drop(vbk::vb_set_error(VB_EDEVICE, "plugin: reading the launch record failed: %s",
                                  hipGetErrorString(e)));
  }
  if (!vbimg::check_launch(rec, err, sizeof err)) return drop(vbk::vb_set_error(VB_EINVAL, "%s", err));
  vb_plugin* p = new (std::nothrow) vb_plugin();
  if (!p) return drop(vbk::vb_set_error(VB_ENOMEM, "out of host memory"));
  p->owner = ctx;
  p->device = device;
  p->module = mod;
  p->function = fn;
  for (int i = 0; i < 3; ++i) p->launch[i] = rec[i];
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_live) g_live = new std::set<const vb_plugin*>();
    g_live->insert(p);
  }
  *out = p;
  return VB_OK;
}

int vb_plugin_info(const vb_plugin* p, int32_t* block, int32_t* rows_per_block, int32_t* dmax) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!live_locked(p)) return vbk::vb_set_error(VB_EINVAL, "not a live vb_plugin handle");
  if (block) *block = p->launch[0];
  if (rows_per_block) *rows_per_block = p->launch[1];
  if (dmax) *dmax = p->launch[2];
  return VB_OK;
}

int vb_plugin_release(vb_plugin* p) {
  if (!p) return VB_OK;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!live_locked(p)) return vbk::vb_set_error(VB_EINVAL, "not a live vb_plugin handle");
    if (--p->refs > 0) return VB_OK;
    g_live->erase(p);
  }
  // the last reference: nothing queued may still run the module's code
  int cur = 0;
  (void)hipGetDevice(&cur);
  int rc = VB_OK;
  if (hipSetDevice(p->device) != hipSuccess) {
    (void)hipGetLastError();
    rc = vbk::vb_set_error(VB_EDEVICE, "plugin release: hipSetDevice(%d) failed", p->device);
  } else {
    // the owning context's stream; a context destroyed first synchronised it then
    if (vbk::ctx_synchronize_if_alive(p->owner) != VB_OK) rc = VB_EDEVICE;
    hipError_t e = hipModuleUnload(p->module);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      rc = vbk::vb_set_error(VB_EDEVICE, "hipModuleUnload failed: %s", hipGetErrorString(e));
    }
    (void)hipSetDevice(cur);
  }
  delete p;
  return rc;
}

}  // extern "C"
