// Host helpers of the translation units behind the C ABI (eqlb_api.hip, eqlb_boundary_setup.hip,
// eqlb_boundary_update.hip, eqlb_sweep.hip, eqlb_tiling_host.hip; they include it through eqlb_handle.h): error return,
// device upload / free and the owner of a device array, the exception barrier of the entry points, set-up profiling.
#pragma once

#include "eqlb_internal.h"

#include <chrono>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <new>
#include <utility>

namespace
{
// EQLB_PROFILE_SETUP=1: wall time of the set-up phases on stderr
struct SetupTimer
{
  bool on;
  std::chrono::steady_clock::time_point t0;
  SetupTimer() : on(getenv("EQLB_PROFILE_SETUP") != nullptr), t0(std::chrono::steady_clock::now()) {}
  void lap(const char* what)
  {
    if (!on)
      return;
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[eqlb setup] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
    t0 = t1;
  }
};

// message of eqlb_last_error (thread-local, eqlb_api.hip) + the code back
template <typename... Args>
int fail(int code, const char* fmt, Args... args)
{
  return eqlb::set_error(code, fmt, args...);
}

#define HIP_TRY(expr)                                                                             \
  do                                                                                              \
  {                                                                                               \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(EQLB_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));                \
  } while (0)

// status of a step of this library: back to the caller unless it is EQLB_OK
#define EQLB_TRY(expr)                                                                             \
  do                                                                                              \
  {                                                                                               \
    if (const int st_ = (expr))                                                                   \
      return st_;                                                                                 \
  } while (0)

template <typename T>
int upload(T** dst, const T* src, size_t n)
{
  *dst = nullptr;
  if (n == 0)
    n = 1;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), n * sizeof(T)));
  if (src)
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
void dfree(T*& p)
{
  if (p)
    (void)hipFree(p);
  p = nullptr;
}
} // namespace


namespace eqlb
{
// A device array and its owner: freed with it, move-only.  Reads as the plain pointer where one is expected.
template <typename T>
class DevBuf
{
  T* p_ = nullptr;

public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    std::swap(p_, o.p_); // (o frees what this one held)
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() { dfree(p_); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  // n elements (at least one), copied from src unless that is nullptr; what the buffer held before is freed first
  int upload(const T* src, size_t n)
  {
    reset();
    return ::upload(&p_, src, n);
  }
  int alloc(size_t n) { return upload(nullptr, n); }
};

// std::vector without value initialisation: the big scratch arrays of the tile builder are written completely by the
// worker threads - a zero fill by the calling thread would touch (page-fault) tens of MB serially first
template <typename T>
struct default_init_alloc : std::allocator<T>
{
  template <typename U>
  struct rebind
  {
    using other = default_init_alloc<U>;
  };
  template <typename U, typename... A>
  void construct(U* p, A&&... a)
  {
    if constexpr (sizeof...(A) == 0)
      ::new (static_cast<void*>(p)) U;
    else
      ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
  }
};
template <typename T>
using uvec = std::vector<T, default_init_alloc<T>>;

} // namespace eqlb

// Nothing may leave an extern "C" entry point as an exception (a ctypes / cgo / JNI caller would be terminated):
// function-try-blocks around the entries that allocate on the host or start worker threads.
#define EQLB_CATCH_ALL                                                                                       \
  catch (const std::bad_alloc&) { return fail(EQLB_ERR_NO_MEMORY, "host memory exhausted"); }                \
  catch (const std::exception& e) { return fail(EQLB_ERR_DEVICE, "internal error: %s", e.what()); }         \
  catch (...) { return fail(EQLB_ERR_DEVICE, "internal error"); }
