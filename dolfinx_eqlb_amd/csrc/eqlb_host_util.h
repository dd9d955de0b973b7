// Host helpers of every translation unit that allocates device memory or stages a host-memory call: error return,
// the owners of device memory (DevBuf, DevCarve, StreamBuf - no other file names the allocator) and of events and
// streams (DevEvent, DevStream - no other file creates or destroys one), the staged host call (HostCall), the exception
// barrier of the entry points, set-up profiling, and the coefficient rules of eqlb_cell_coeff.h (which it includes) as
// refusals of an entry point.  Host code only.  Included
//   through eqlb_mesh_handle.h (the units that dereference a mesh handle)
//     and eqlb_handle.h by eqlb_api.hip, eqlb_boundary_setup.hip, eqlb_boundary_update.hip, eqlb_sweep.hip,
//       eqlb_tiling_host.hip, eqlb_bc_carry.hip,
//     and eqlb_refine_plan.h by eqlb_mesh_refine.hip, eqlb_transfer.hip, eqlb_bc_carry.hip, eqlb_multilevel.hip,
//     directly by eqlb_mesh_build.hip, eqlb_marking.hip, eqlb_primal_flux.hip, eqlb_primal_solve.hip,
//   through eqlb_coarse.h by eqlb_coarse.hip, eqlb_multilevel.hip,
//   through eqlb_estimate_kernels.h by eqlb_estimate.hip, eqlb_estimate_lowdeg.hip, eqlb_estimate_lowdeg_k4.hip,
//   directly by eqlb_tiling_device.hip, eqlb_halo_rccl.hip.
#pragma once

#include "eqlb_cell_coeff.h"
#include "eqlb_internal.h"

#include <chrono>
#include <memory>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <initializer_list>
#include <new>
#include <utility>
#include <vector>

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
  void reset()
  {
    if (p_)
      (void)hipFree(p_);
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  // n elements (at least one), copied from src unless that is nullptr; what the buffer held before is freed first
  int upload(const T* src, size_t n)
  {
    reset();
    if (n == 0)
      n = 1;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)));
    if (src)
      HIP_TRY(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  int alloc(size_t n) { return upload(nullptr, n); }
  // the same without a message: n elements (at least one), for callers that word their own error
  hipError_t alloc_raw(size_t n)
  {
    reset();
    return hipMalloc(reinterpret_cast<void**>(&p_), (n ? n : 1) * sizeof(T));
  }
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


// blocks of `threads` that cover n items
inline unsigned grid_of(int64_t n, int threads = 256) { return (unsigned)((n + threads - 1) / threads); }

// bytes up to the next multiple of 256: the alignment of the pieces of a carved allocation
inline size_t round_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the memory space of a call is one of the two the ABI names
inline int check_memspace(const char* who, int32_t memspace)
{
  if (memspace != EQLB_MEM_DEVICE && memspace != EQLB_MEM_HOST)
    return fail(EQLB_ERR_INVALID_ARGUMENT, "%s: unknown memory space", who);
  return EQLB_OK;
}

// ---- the coefficient rules of eqlb_cell_coeff.h as refusals of an entry point ---------------------------------------
namespace
{
// entry i of a breaks the rule of c
inline int fail_cell(const char* who, const CellCoeff& c, const double* a, long long i)
{
  char msg[256];
  format_cell(msg, sizeof(msg), who, c, a, i);
  return fail(EQLB_ERR_INVALID_ARGUMENT, "%s", msg);
}

// a scalar, checked where no array takes its place
inline int check_scalar(const char* who, const char* name, const ScalarRule& rule, double x)
{
  if (rule.ok(x))
    return EQLB_OK;
  char msg[256];
  format_scalar(msg, sizeof(msg), who, name, rule, x);
  return fail(EQLB_ERR_INVALID_ARGUMENT, "%s", msg);
}

// HOST arrays of n cells (nullptr: not given): the first CELL that breaks a rule is refused, and within it the array
// that stands first
struct CellArray
{
  const CellCoeff& coeff;
  const double* a;
};
inline int check_cells(const char* who, long long n, std::initializer_list<CellArray> arrays)
{
  const CellArray* worst = nullptr;
  long long at = n;
  for (const CellArray& x : arrays)
    if (const long long i = x.a ? x.coeff.first_bad(x.a, at) : -1; i >= 0)
    {
      worst = &x;
      at = i; // (the arrays behind this one are read up to this cell only)
    }
  return worst ? fail_cell(who, worst->coeff, worst->a, at) : EQLB_OK;
}
} // namespace

// One device allocation carved into typed pieces: declare the pieces, alloc() once, read the pointers back from the
// pieces.  Every piece starts on a multiple of 256 bytes; one of length zero is allowed.  Not movable (the pieces
// point back at it).  A piece reads as nullptr until alloc(): keep it (auto) and let it convert where it is used.
class DevCarve;
template <typename T>
struct DevPiece
{
  const DevCarve* owner = nullptr; // nullptr: no such piece, reads as nullptr
  size_t off = 0;
  inline T* get() const;
  operator T*() const { return get(); }
  DevPiece at(size_t i) const { return {owner, off + i * sizeof(T)}; } // the piece from element i on
};

class DevCarve
{
  DevBuf<char> buf_;
  size_t bytes_ = 0;

public:
  DevCarve() = default;
  DevCarve(const DevCarve&) = delete;
  DevCarve& operator=(const DevCarve&) = delete;
  template <typename T>
  DevPiece<T> piece(size_t n)
  {
    DevPiece<T> p{this, bytes_};
    bytes_ += round_up256(n * sizeof(T));
    return p;
  }
  hipError_t alloc() { return buf_.alloc_raw(bytes_); }
  char* base() const { return buf_.get(); }
  size_t bytes() const { return bytes_; }
};

template <typename T>
inline T* DevPiece<T>::get() const
{
  return (owner && owner->base()) ? reinterpret_cast<T*>(owner->base() + off) : nullptr;
}

// Work space of a device-memory call that must not wait: taken from the stream-ordered allocator and given back in
// stream order when the owner ends.
class StreamBuf
{
  void* p_ = nullptr;
  hipStream_t stream_ = nullptr;

public:
  StreamBuf() = default;
  StreamBuf(const StreamBuf&) = delete;
  StreamBuf& operator=(const StreamBuf&) = delete;
  ~StreamBuf()
  {
    if (p_)
      (void)hipFreeAsync(p_, stream_);
  }
  hipError_t alloc(size_t bytes, hipStream_t stream)
  {
    stream_ = stream;
    return hipMallocAsync(&p_, bytes, stream);
  }
  template <typename T>
  T* as() const
  {
    return static_cast<T*>(p_);
  }
};

// An event / a stream and its owner: created with the given flags, destroyed with the owner, move-only.  Reads as the
// plain handle (nullptr until create()); no other file names the calls that create or destroy one.
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class DevHandle
{
  H h_ = nullptr;

public:
  DevHandle() = default;
  DevHandle(DevHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  DevHandle& operator=(DevHandle&& o) noexcept
  {
    std::swap(h_, o.h_); // (o destroys what this one held)
    return *this;
  }
  ~DevHandle()
  {
    if (h_)
      (void)Destroy(h_);
  }
  hipError_t create(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
  operator H() const { return h_; }
};
using DevEvent = DevHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using DevStream = DevHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// A host-memory call: the same work as the device-memory call, staged and synchronous.  Declare the arrays (a null
// host pointer stays null), upload(stream) allocates once and sends the inputs on the caller's stream, the entry point
// runs what its device branch runs on the pieces, finish(stream) enqueues the copies back on the same stream, waits for
// it once and returns the first error seen anywhere.  An output whose length is known only after the run: out_prefix
// after the first finish, then finish again.
class HostCall
{
  struct Copy
  {
    void* host;
    size_t off, bytes;
  };
  DevCarve mem_;
  std::vector<Copy> ins_, outs_;
  hipError_t err_ = hipSuccess;

public:
  template <typename T>
  DevPiece<T> in(const T* host, size_t n)
  {
    if (!host)
      return {};
    const DevPiece<T> p = mem_.piece<T>(n);
    ins_.push_back({const_cast<T*>(host), p.off, n * sizeof(T)});
    return p;
  }
  template <typename T>
  DevPiece<T> out(T* host, size_t n)
  {
    if (!host)
      return {};
    const DevPiece<T> p = mem_.piece<T>(n);
    outs_.push_back({host, p.off, n * sizeof(T)});
    return p;
  }
  template <typename T>
  DevPiece<T> scratch(size_t n)
  {
    return mem_.piece<T>(n);
  }
  // the first n elements of a piece, copied back by the next finish
  template <typename T>
  void out_prefix(T* host, const DevPiece<T>& p, size_t n)
  {
    outs_.push_back({host, p.off, n * sizeof(T)});
  }
  // an error of the run between upload and finish
  void note(hipError_t e)
  {
    if (err_ == hipSuccess)
      err_ = e;
  }
  hipError_t upload(hipStream_t stream)
  {
    note(mem_.alloc());
    for (const Copy& c : ins_)
      if (err_ == hipSuccess && c.bytes)
        note(hipMemcpyAsync(mem_.base() + c.off, c.host, c.bytes, hipMemcpyHostToDevice, stream));
    return err_;
  }
  hipError_t finish(hipStream_t stream)
  {
    for (const Copy& c : outs_)
      if (err_ == hipSuccess && c.bytes)
        note(hipMemcpyAsync(c.host, mem_.base() + c.off, c.bytes, hipMemcpyDeviceToHost, stream));
    outs_.clear();
    if (mem_.base())
      note(hipStreamSynchronize(stream)); // (also after an error: the allocation ends with this object)
    return err_;
  }
};

} // namespace eqlb

// Nothing may leave an extern "C" entry point as an exception (a ctypes / cgo / JNI caller would be terminated):
// function-try-blocks around the entries that allocate on the host or start worker threads.
#define EQLB_CATCH_ALL                                                                                       \
  catch (const std::bad_alloc&) { return fail(EQLB_ERR_NO_MEMORY, "host memory exhausted"); }                \
  catch (const std::exception& e) { return fail(EQLB_ERR_DEVICE, "internal error: %s", e.what()); }         \
  catch (...) { return fail(EQLB_ERR_DEVICE, "internal error"); }
