// device_buf.h -- the library's error types, the HIP_OK check and the owning buffers of the host side (engine.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace elemdp {

struct HipError : std::runtime_error {
  explicit HipError(const std::string& m) : std::runtime_error(m) {}
};
struct ArgError : std::runtime_error {
  explicit ArgError(const std::string& m) : std::runtime_error(m) {}
};
struct StateError : std::runtime_error {
  explicit StateError(const std::string& m) : std::runtime_error(m) {}
};

#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

inline size_t free_device_bytes() {
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  return free_b;
}

// owning device buffer
class DevBuf {
 public:
  DevBuf() = default;
  ~DevBuf() { reset(); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  // (an allocation that is large enough and at most twice too large is kept: fresh device memory costs ~20 ms / GB, and
  // the plan sets of a load are rebuilt chunk after chunk with similar sizes; bytes() is the capacity)
  // slack: allocate an eighth more than asked for -- buffers whose size depends on the data (interior-loop items of a batch):
  // the next batch of the same shape then fits without a re-allocation
  // (such a buffer is also never given up for a smaller one: the last chunk of a load is smaller than the others)
  // returns true when the memory is fresh (its contents undefined), false when the buffer was kept
  bool alloc(size_t bytes, bool slack = false) {
    bytes = bytes ? bytes : 8;
    if (p_ && bytes <= bytes_ && (slack || bytes_ <= 2 * bytes + (size_t(1) << 20))) return false;
    reset();
    bytes_ = slack ? bytes + bytes / 8 : bytes;
    HIP_OK(hipMalloc(&p_, bytes_));
    return true;
  }
  void reset() { if (p_) { (void)hipFree(p_); p_ = nullptr; bytes_ = 0; } }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
  template <class T> void upload(const std::vector<T>& v, hipStream_t st) {
    alloc(v.size() * sizeof(T));
    if (!v.empty()) HIP_OK(hipMemcpyAsync(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// pinned host staging buffer, kept from load to load (a fresh std::vector of 24 MB costs its page faults -- 30 ms per
// 10 000 x L=300 for the staging arrays of load_batch -- and a pageable upload goes through the runtime's own staging copies)
class HostBuf {
 public:
  HostBuf() = default;
  ~HostBuf() { if (p_) (void)hipHostFree(p_); }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  template <class T> T* get(size_t n) {
    const size_t bytes = std::max<size_t>(n * sizeof(T), 8);
    if (bytes > bytes_) {
      if (p_) (void)hipHostFree(p_);
      p_ = nullptr; bytes_ = 0;
      void* p = nullptr;   // (p_ and bytes_ are set once the allocation has succeeded)
      HIP_OK(hipHostMalloc(&p, bytes + bytes / 8, hipHostMallocDefault));
      p_ = p; bytes_ = bytes + bytes / 8;
    }
    return static_cast<T*>(p_);
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace elemdp
