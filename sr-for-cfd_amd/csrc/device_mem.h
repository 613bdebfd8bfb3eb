// Owners of HIP resources (not part of the C ABI; included by engine.h, which defines HIPCHECK).  A struct holds its device memory,
// page-locked memory, streams, events and graph executables as these; the member's destructor is the only release, so no teardown
// lists them again and no early return leaks one or frees one twice.  The struct's own destructor only selects the device first.
#pragma once

namespace srcfd {

// Move-only owner of one allocation of n elements of T: hipMalloc / hipFree, or hipHostMalloc / hipHostFree when PINNED.
template <class T, bool PINNED = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { (void)release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DevBuf() { (void)release(); }
  // frees and forgets the allocation whether or not the free succeeded
  int release() {
    T* p = p_;
    p_ = nullptr; n_ = 0;
    if (p) HIPCHECK(PINNED ? hipHostFree(p) : hipFree(p));
    return SRCFD_OK;
  }
  // releases what it holds, then allocates n elements (uninitialised)
  int alloc(size_t n) {
    int rc = release();
    if (rc) return rc;
    if (PINNED) HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), hipHostMallocDefault));
    else HIPCHECK(hipMalloc(&p_, n * sizeof(T)));
    n_ = n;
    return SRCFD_OK;
  }
  // alloc + synchronous copy from the host; nothing to upload leaves the buffer empty
  int upload(const T* src, size_t n) {
    int rc = n ? alloc(n) : release();
    if (rc || !n) return rc;
    HIPCHECK(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
    return SRCFD_OK;
  }
  int upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <class T> using PinnedBuf = DevBuf<T, true>;

// Move-only owner of a stream, an event or a graph executable.  The owner creates it where it needs it (hipStreamCreateWithFlags(s.out(), ...));
// the destructor, reset() and a second out() destroy it.
template <class H, hipError_t (*DESTROY)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h_) (void)DESTROY(h_);
    h_ = nullptr;
  }
  H* out() { reset(); return &h_; }
  operator H() const { return h_; }   // the HIP calls and kernel launches take the handle as it is

 private:
  H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace srcfd
