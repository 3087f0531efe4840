"""The owners of HIP resources (nim_groth16_amd/csrc/hip_owners.hpp) hold what the host layer relies on: compiled with
the HOST compiler against the ROCm headers, compile-time only (no GPU, no runtime library, nothing is linked)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nim_groth16_amd", "csrc")

CHECKS = r"""
#include "hip_owners.hpp"
#include <string>
#include <utility>
#include <vector>

template <class Owner, class Raw>
constexpr bool thin_move_only() {
  return !std::is_copy_constructible<Owner>::value && !std::is_copy_assignable<Owner>::value &&
         std::is_nothrow_move_constructible<Owner>::value && std::is_nothrow_move_assignable<Owner>::value &&
         std::is_nothrow_default_constructible<Owner>::value && !std::has_virtual_destructor<Owner>::value &&
         sizeof(Owner) == sizeof(Raw);
}
static_assert(thin_move_only<DevMem<>, void*>(), "DevMem<>");
static_assert(thin_move_only<DevMem<unsigned>, unsigned*>(), "DevMem<T>");
static_assert(thin_move_only<PinnedMem<unsigned char>, unsigned char*>(), "PinnedMem");
static_assert(thin_move_only<Event, hipEvent_t>(), "Event");
static_assert(thin_move_only<Stream, hipStream_t>(), "Stream");
// the raw handle comes back unchanged, and an empty owner is false
static_assert(std::is_same<decltype(std::declval<Event&>().get()), hipEvent_t>::value, "Event::get");
static_assert(std::is_same<decltype(std::declval<Stream&>().get()), hipStream_t>::value, "Stream::get");
static_assert(std::is_same<decltype(std::declval<DevMem<unsigned>&>().get()), unsigned*>::value, "DevMem::get");
static_assert(std::is_constructible<bool, Event>::value, "explicit operator bool");
// the creation helpers are checked like any HIP call
static_assert(std::is_same<decltype(dev_alloc(std::declval<DevMem<>&>(), 1)), hipError_t>::value, "dev_alloc");
static_assert(std::is_same<decltype(pinned_alloc(std::declval<PinnedMem<>&>(), 1)), hipError_t>::value, "pinned_alloc");
static_assert(std::is_same<decltype(event_create(std::declval<Event&>())), hipError_t>::value, "event_create");
static_assert(std::is_same<decltype(stream_create(std::declval<Stream&>())), hipError_t>::value, "stream_create");

// a record of owners (the pool's PoolRec, the context's ProfEntry) lives in a std::vector that grows by moving
struct Rec {
  DevMem<> mem;
  Event up, done;
};
static_assert(std::is_nothrow_move_constructible<Rec>::value && !std::is_copy_constructible<Rec>::value, "Rec");
static_assert(sizeof(Rec) == 3 * sizeof(void*), "Rec");
void grow(std::vector<Rec>& v) { v.resize(v.size() + 1); }

// a half-built object is destroyed by its own destroy function
struct Obj {
  int x;
};
void obj_destroy(Obj*);
static_assert(thin_move_only<Building<Obj, obj_destroy>, Obj*>(), "Building");
"""


def test_owner_types_are_thin_and_move_only(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    assert os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")), "ROCm headers not found"
    src = tmp_path / "owners_check.cpp"
    src.write_text(CHECKS)
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
                        "-Wall", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_raw_release_calls_live_in_the_owner_header_only():
    """hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy appear in hip_owners.hpp and nowhere else"""
    import re
    pat = re.compile(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy)\b")
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cuh", ".hpp", ".inc")) and name != "hip_owners.hpp":
            with open(os.path.join(CSRC, name)) as f:
                hits += [f"{name}:{i}" for i, line in enumerate(f, 1) if pat.search(line)]
    assert not hits, hits
