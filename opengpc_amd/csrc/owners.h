// owners.h -- move-only owners of what the host code allocates: memory blocks, streams, events.  Plain C++, no HIP header:
// the allocating and releasing calls come from a backend (template parameter), so gpc_hip.hip instantiates the owners over
// the HIP runtime and a stand-alone program drives them with a counting fake under the sanitizers (tests/cpp/owners_check.cpp).
//
// The owners are dumb: they never wait for a stream.  Whoever frees a block that queued work may still use waits first.
#pragma once
#include <cstddef>

namespace gpc {

// `cap` bytes at `p`.  B: `status` (an integer or enum, 0 = done), `static status alloc(void** p, size_t bytes, unsigned flags)`,
// `static status release(void* p, size_t bytes)`.
template <class B, class T = void>
struct Block {
  using status = typename B::status;
  T* p = nullptr;
  size_t cap = 0;

  Block() = default;
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  Block(Block&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Block& operator=(Block&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~Block() { (void)reset(); }

  // releases what the owner holds (nothing: no call); the owner is empty afterwards, whatever the backend answers
  status reset() {
    if (!p) return status();
    void* q = p;
    const size_t n = cap;
    p = nullptr, cap = 0;
    return B::release(q, n);
  }
  // a new block of exactly `bytes` in place of what the owner holds; empty with cap == 0 where either call fails
  status alloc(size_t bytes, unsigned flags = 0) {
    status e = reset();
    if (e != status()) return e;
    void* q = nullptr;
    e = B::alloc(&q, bytes, flags);
    if (e != status()) return e;
    p = static_cast<T*>(q), cap = bytes;
    return e;
  }
};

// A stream or an event.  B: `handle` (a pointer type), `status`, `static status create(handle* h, unsigned flags)`,
// `static status destroy(handle h)`.  Converts to the bare handle, so it is passed to the runtime as one.
template <class B>
struct Handle {
  using handle = typename B::handle;
  using status = typename B::status;
  handle h = handle();

  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = handle(); }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      (void)reset();
      h = o.h;
      o.h = handle();
    }
    return *this;
  }
  ~Handle() { (void)reset(); }
  operator handle() const { return h; }

  status reset() {
    if (!h) return status();
    const handle q = h;
    h = handle();
    return B::destroy(q);
  }
  status create(unsigned flags) {
    status e = reset();
    if (e != status()) return e;
    handle q = handle();
    e = B::create(&q, flags);
    if (e == status()) h = q;
    return e;
  }
};

}  // namespace gpc
