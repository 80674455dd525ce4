// Stand-alone check of the host helpers of csrc/gnr_host.h (gnr::Refuse, the limits, gnr::Carve) for a sanitizer build; links nothing
// of the library and touches no device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I${ROCM_PATH:-/opt/rocm}/include \
//       tools/host_layer_check.cpp -o /tmp/host_layer_check && /tmp/host_layer_check
#include <assert.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../graspnerf_amd/csrc/gnr_host.h"

static std::string g_text;
extern "C" int gnr_internal_fail(int code, const char* what, int) { g_text = what; return code; }
extern "C" int gnr_internal_timing_open(const char*, void*) { return -1; }
extern "C" void gnr_internal_timing_close(int, void*) {}

template <typename A, typename B, typename C3>
static size_t carve(void* base, size_t na, size_t nb, size_t nc, A** a, B** b, C3** c) {
    gnr::Carve k(base);
    *a = k.take<A>(na); *b = k.take<B>(nb); *c = k.take<C3>(nc);
    return k.total();
}

int main() {
    const gnr::Refuse no{"gnr_some_entry_fwd"};
    assert(no(GNR_ERR_SHAPE, "max_n must be >= 1") == GNR_ERR_SHAPE && g_text == "gnr_some_entry_fwd: max_n must be >= 1");
    const std::string longest(400, 'x');                      // longer than the local buffer: truncated, never overrun
    assert(no(GNR_ERR_ARG, longest.c_str()) == GNR_ERR_ARG && g_text.size() == 255 && g_text.compare(0, 20, "gnr_some_entry_fwd: ") == 0);
    for (int B : {1, 65535}) assert(gnr::check_scenes(no, GNR_ERR_ARG, B) == GNR_OK);
    for (int B : {0, -1, 65536}) assert(gnr::check_scenes(no, GNR_ERR_ARG, B) == GNR_ERR_ARG && g_text == "gnr_some_entry_fwd: B must be in 1..65535");
    for (int R : {2, 256}) assert(gnr::check_lattice(no, GNR_ERR_SHAPE, R) == GNR_OK);
    for (int R : {1, 0, 257}) assert(gnr::check_lattice(no, GNR_ERR_SHAPE, R) == GNR_ERR_SHAPE && g_text == "gnr_some_entry_fwd: R must be in 2..256");

    int* a; unsigned char* b; double* c;
    const size_t na = 1, nb = 257, nc = 33;
    const size_t total = carve((void*)nullptr, na, nb, nc, &a, &b, &c);               // sizing: no base, every region null
    assert(!a && !b && !c && total == 256 + 512 + 512);
    std::vector<char> heap(total + 256);
    char* base = (char*)(((uintptr_t)heap.data() + 255) & ~(uintptr_t)255);
    assert(carve(base, na, nb, nc, &a, &b, &c) == total);
    assert((char*)a == base && (char*)b == base + 256 && (char*)c == base + 768);
    memset(a, 1, na * sizeof *a); memset(b, 2, nb * sizeof *b); memset(c, 3, nc * sizeof *c);      // every region is the caller's to the last byte
    assert(base[total - 1] == 0 && base[768 + nc * sizeof(double) - 1] == 3);
    return 0;
}
