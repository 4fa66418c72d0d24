// fjgpu_api_common.h -- what the translation units behind the C ABI of libfjgpu.so share (fjgpu_api.hip and fjgpu_frame.hip: entry
// points that take a fjgpu_scene, whose record is fjgpu_scene.h; fjgpu_image_api.hip: entry points that take only buffers): the error
// return, HIP_TRY and transient device buffers.
#ifndef FJGPU_API_COMMON_H
#define FJGPU_API_COMMON_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fjgpu.h"

namespace fjgpu {

// sets the calling thread's fjgpu_last_error() text and returns `code`.  Defined in fjgpu_api.hip, beside the one thread_local string
// of the library.
int fail(int code, const std::string &msg);

struct DeviceBuffers {
  std::vector<void *> ptrs;
  size_t bytes = 0;
  ~DeviceBuffers() { for (void *p : ptrs) (void) hipFree(p); }
  template <class T> int upload(const T *src, size_t n, const T **out)
  {
    *out = nullptr;
    if (n == 0 || src == nullptr) return 0;
    void *d = nullptr;
    if (hipMalloc(&d, n * sizeof(T)) != hipSuccess) return -1;
    ptrs.push_back(d);
    bytes += n * sizeof(T);
    if (hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return -1;
    *out = static_cast<const T *>(d);
    return 0;
  }
  template <class T> int alloc(size_t n, T **out)
  {
    void *d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return -1;
    ptrs.push_back(d);
    bytes += std::max<size_t>(n, 1) * sizeof(T);
    *out = static_cast<T *>(d);
    return 0;
  }
};

}  // namespace fjgpu

// (the message carries the expression's text: keep its spelling where the macro is used)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
  return fjgpu::fail(FJGPU_ENODEV, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

#endif
