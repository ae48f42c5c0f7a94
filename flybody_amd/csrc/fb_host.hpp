// Host-only plumbing of libflybody_hip.so, included by fb_engine.hip behind the HIP (or emulation) header: the error message of the
// C-ABI (fb_last_error) and the two owners of device resources.  Every device block the engine allocates is a DevBuf and every event a
// DevEvent -- members of fb_batch, or locals on the way there -- so nothing is freed by hand, a failed call gives back what it had
// allocated so far, and hipMalloc / hipFree appear in this file only.  Nothing more than that: no pools, no allocator interface, no
// reference counts.
#pragma once
#include <exception>
#include <string>
#include <type_traits>
#include <utility>

static thread_local std::string g_err;
static int fail(const std::string& s) { g_err = s; return -1; }

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// an exception of the host code (a model accessor, std::bad_alloc) becomes the entry point's error return
#define FB_GUARD_BEGIN try {
#define FB_GUARD_END } catch (const std::exception& e_) { return fail(e_.what()); }

// Move-only owner of one device block of n elements T; T = void: n bytes (the buffers whose element type follows the batch's precision).
// The allocating calls return 0, or -1 with the message set as HIPCHK sets it, and then leave the buffer EMPTY.  None of them
// synchronises: a caller that replaces a block a launch may still read waits for the device first, where it did before.
template <typename T>
class DevBuf {
  T* p_ = nullptr; size_t n_ = 0;
  static constexpr size_t elem() { if constexpr (std::is_void<T>::value) return 1; else return sizeof(T); }
  int failed(const char* what, size_t n, hipError_t e) {
    (void)hipGetLastError();                           // (the failure is reported here: a later launch's check must not meet it again)
    reset();
    return fail(std::string(what) + " of " + std::to_string(n*elem()) + " bytes: " + hipGetErrorString(e));
  }
public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  size_t count() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }
  // a new block of n elements, contents undefined (what the buffer held is freed first)
  int alloc(size_t n) {
    reset();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, n*elem());
    if (e != hipSuccess) return failed("hipMalloc", n, e);
    p_ = (T*)p; n_ = n;
    return 0;
  }
  int alloc_zeroed(size_t n) {
    if (alloc(n)) return -1;
    const hipError_t e = hipMemset(p_, 0, n*elem());
    return e == hipSuccess ? 0 : failed("hipMemset", n, e);
  }
  // at least n elements: a block that is large enough stays as it is, otherwise a new one (contents NOT kept); *grew says which
  int reserve(size_t n, bool* grew = nullptr) {
    const bool need = !p_ || n_ < n;
    if (grew) *grew = need;
    return need ? alloc(n) : 0;
  }
};

// The same ownership for an event.
class DevEvent {
  hipEvent_t e_ = nullptr;
public:
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  DevEvent(DevEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~DevEvent() { reset(); }
  void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
  hipEvent_t get() const { return e_; }
  explicit operator bool() const { return e_ != nullptr; }
  int create() {
    reset();
    const hipError_t e = hipEventCreate(&e_);
    if (e != hipSuccess) { e_ = nullptr; (void)hipGetLastError(); return fail(std::string("hipEventCreate: ") + hipGetErrorString(e)); }
    return 0;
  }
};
