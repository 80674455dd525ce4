// Host layer shared by every source file of libgnr.so: the one error text, an entry point's refusals, the batch and lattice limits,
// the workspace carve, the per-launch timing bracket and the one way to launch a kernel.  Internal (not installed next to
// include/gnr.h), host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <atomic>

#include "../../include/gnr.h"

// Defined in gnr_capi.inc, next to the thread's error text (gnr_last_error) and the process-wide timing state (gnr_timing_*); not
// part of the public ABI.  gnr_internal_timing_open returns the slot of the opened bracket, or -1 when the launch is not bracketed.
extern "C" int gnr_internal_fail(int code, const char* what, int hip_error);
extern "C" int gnr_internal_timing_open(const char* label, void* stream);
extern "C" void gnr_internal_timing_close(int idx, void* stream);

namespace gnr {

// Every refusal and every HIP error of the library: `what`, or "what: hipGetErrorString(e)", becomes the calling thread's
// gnr_last_error() text; returns `code`.
static inline int fail(int code, const char* what, hipError_t e = hipSuccess) { return gnr_internal_fail(code, what, (int)e); }
#define GNR_HIP(call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) return gnr::fail(GNR_ERR_HIP, #call, e_);       \
    } while (0)

// An entry point's refusals: `gnr::Refuse no{"gnr_x_fwd"};` then `return no(code, what)` fails with the text "gnr_x_fwd: what".
struct Refuse {
    const char* fn;
    int operator()(int code, const char* what) const {
        char text[256];                                // (fail() copies the text)
        snprintf(text, sizeof text, "%s: %s", fn, what);
        return fail(code, text);
    }
};

// The limits every volume operator shares: the scene is a grid dimension (y or z: 65535 at most), a lattice has 2..256 voxels a side.
// check_*: GNR_OK, or the refusal under the entry point's own status code.
constexpr int MAX_SCENES = 65535, MIN_LATTICE = 2, MAX_LATTICE = 256;
static inline bool scenes_ok(int B) { return B >= 1 && B <= MAX_SCENES; }
static inline bool lattice_ok(int R) { return R >= MIN_LATTICE && R <= MAX_LATTICE; }
static inline int check_scenes(const Refuse& no, int code, int B) { return scenes_ok(B) ? GNR_OK : no(code, "B must be in 1..65535"); }
static inline int check_lattice(const Refuse& no, int code, int R) { return lattice_ok(R) ? GNR_OK : no(code, "R must be in 2..256"); }

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// A workspace, carved in order into regions aligned to 256 bytes.  An operator states its regions once, in one function over a
// Carve: its *_workspace_bytes carves nullptr (every take() is null) and returns total(), its entry point carves the caller's pointer.
struct Carve {
    char* base; size_t off;
    explicit Carve(void* ws) : base((char*)ws), off(0) {}
    template <typename T> T* take(size_t count) { T* q = base ? (T*)(base + off) : nullptr; off += al256(count * sizeof(T)); return q; }
    size_t total() const { return off; }
};

// hipFuncSetAttribute (dynamic LDS above 64 KiB) is per device: one bit per device id and kernel (launch())
static inline bool attr_needed(std::atomic<unsigned long long>& done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return true;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load() & bit) return false;
    done.fetch_or(bit);
    return true;
}

// A pair of HIP events on `stream` around whatever is enqueued while the scope lives, reported under `label` between
// gnr_timing_begin() and gnr_timing_end().  label == nullptr: never bracketed.
struct TimingScope {
    void* st; int idx;
    TimingScope(const char* label, void* stream) : st(stream), idx(label ? gnr_internal_timing_open(label, stream) : -1) {}
    ~TimingScope() { if (idx >= 0) gnr_internal_timing_close(idx, st); }
    TimingScope(const TimingScope&) = delete;
    TimingScope& operator=(const TimingScope&) = delete;
};

#ifdef __HIPCC__      // (gnr_pack.cpp and gnr_host_rng.cpp are plain C++: they fail() like every other file and launch nothing)
// Every kernel launch of the library: the timing bracket around the launch alone, then the launch's own error check (the text names
// the label, or the kernel when there is none).  A kernel that takes more dynamic LDS than a launch gets by default names its maximum
// as MAX_LDS -- the most any launch of it asks for, not this launch's bytes -- and has hipFuncAttributeMaxDynamicSharedMemorySize
// raised to it on the first launch per device (one static per kernel).
// A kernel passed as a template argument has lost its default arguments: the call sites spell them out.
template <auto Kernel, size_t MAX_LDS = 0, typename... Args>
static int launch(const char* label, hipStream_t st, dim3 grid, dim3 block, size_t lds_bytes, Args... args) {
    if constexpr (MAX_LDS != 0) {
        static std::atomic<unsigned long long> attr_done{0};
        if (attr_needed(attr_done)) GNR_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS));
    }
    { TimingScope ts(label, st); hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...); }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GNR_OK : fail(GNR_ERR_HIP, label ? label : __PRETTY_FUNCTION__, e);
}
#endif

}  // namespace gnr
