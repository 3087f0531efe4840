// Move-only owners of the four HIP resource kinds the host layer holds: device memory, pinned host memory, events and
// streams.  Each is a std::unique_ptr with a stateless deleter: the size of the raw handle, empty = owns nothing, no
// reference counting.  The raw handle (`.get()`) is what every HIP call and kernel launch takes.  Includable on its
// own (tests/test_host_owners_cpu.py compiles it with the host compiler).
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <type_traits>

struct DevFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
struct HostFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
struct EventDestroy {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct StreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
template <class T = void>
using DevMem = std::unique_ptr<T, DevFree>;
template <class T = void>
using PinnedMem = std::unique_ptr<T, HostFree>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// Creation into an owner (what it held before is released).  They return the hipError_t of the one HIP call they make,
// so that a caller checks them like any other HIP call; allocations bind to the calling thread's current device.
template <class T>
inline hipError_t dev_alloc(DevMem<T>& out, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  out.reset(static_cast<T*>(p));
  return e;
}
template <class T>
inline hipError_t pinned_alloc(PinnedMem<T>& out, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  out.reset(static_cast<T*>(p));
  return e;
}
inline hipError_t event_create(Event& out, unsigned flags = hipEventDisableTiming) {
  hipEvent_t ev = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&ev, flags);
  out.reset(ev);
  return e;
}
inline hipError_t stream_create(Stream& out, unsigned flags = hipStreamNonBlocking) {
  hipStream_t s = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&s, flags);
  out.reset(s);
  return e;
}

// A half-built C-ABI object: destroyed by its own destroy function on every early return, released into *out on success.
template <class T, void (*Destroy)(T*)>
struct DestroyWith {
  void operator()(T* p) const { Destroy(p); }
};
template <class T, void (*Destroy)(T*)>
using Building = std::unique_ptr<T, DestroyWith<T, Destroy>>;
