// thread_cache_check.cpp -- the bookkeeping of csrc/thread_cache.h (ThreadCache over Arena) on the host, with the HIP allocation calls
// replaced by malloc / free that keep a ledger: built with g++ -fsanitize=address,undefined and run by tests/test_thread_cache_cpu.py.
// Two std::threads each drive two instances (as ingest.hip and segment.hip keep one each) through begin / take / staging growth /
// trim, twice over.  Checked: an instance's arenas and pinned block are its own, a warm round allocates nothing, the pinned block
// grows by the one rule and only when it must, trim gives back exactly what the instance took and a second trim is a no-op, a device
// id < 0 resolves to the thread's current device, and at the end every block of every thread has been freed (the sanitizer's leak
// check says the same of the std::map).
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>

static std::atomic<long long> g_live_dev(0), g_live_pin(0), g_failed(0);
static thread_local int tl_device = 0;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "thread_cache_check: line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

static hipError_t stub_malloc(void** p, size_t bytes) { *p = malloc(bytes); memset(*p, 0xA5, bytes < 64 ? bytes : 64); ++g_live_dev; return *p ? hipSuccess : hipErrorOutOfMemory; }
static hipError_t stub_free(void* p) { if (p) --g_live_dev; free(p); return hipSuccess; }
static hipError_t stub_host_malloc(void** p, size_t bytes, unsigned) { *p = malloc(bytes); memset(*p, 0x5A, bytes); ++g_live_pin; return *p ? hipSuccess : hipErrorOutOfMemory; }
static hipError_t stub_host_free(void* p) { if (p) --g_live_pin; free(p); return hipSuccess; }
static hipError_t stub_get_device(int* d) { *d = tl_device; return hipSuccess; }
static hipError_t stub_sync(hipStream_t) { return hipSuccess; }
static const char* stub_error_string(hipError_t) { return "stub"; }
#define hipMalloc stub_malloc
#define hipFree stub_free
#define hipHostMalloc stub_host_malloc
#define hipHostFree stub_host_free
#define hipGetDevice stub_get_device
#define hipStreamSynchronize stub_sync
#define hipGetErrorString stub_error_string
#define hipGetLastError() hipSuccess

#include "../../model_matching_amd/csrc/thread_cache.h"

namespace stocs {
unsigned long long g_dev_allocs = 0;
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }
}  // namespace stocs
using namespace stocs;

static thread_local ThreadCache tl_a, tl_b;   // as ingest.hip's and segment.hip's

static unsigned long long allocs() { return __atomic_load_n(&g_dev_allocs, __ATOMIC_RELAXED); }

// one call of an entry point: the arena of `device`, a few regions, the staging block written end to end
static void call(ThreadCache& c, int device, size_t region, size_t stage) {
    Arena* a = NULL;
    CHECK(c.begin(device, &a) == STOCS_OK && a == c.cur && c.dev == (device < 0 ? tl_device : device));
    char* p[3] = {NULL, NULL, NULL};
    for (int k = 0; k < 3; ++k) { CHECK(a->take(region * (k + 1), (void**)&p[k]) == STOCS_OK); memset(p[k], k, region * (k + 1)); }
    CHECK(p[0] != p[1] && p[1] != p[2] && ((size_t)(p[1] - p[0]) >= region || (size_t)(p[0] - p[1]) >= 2 * region));
    char* pin = NULL;
    CHECK(c.staging(stage, &pin) == STOCS_OK && pin == (char*)c.pin && c.pin_bytes >= stage);
    memset(pin, 7, stage);
}

static void worker(int id) {
    tl_device = id;
    for (int round = 0; round < 2; ++round) {
        CHECK(!tl_a.ws && !tl_a.pin && !tl_b.ws && !tl_b.pin && tl_a.pin_bytes == 0);
        call(tl_a, -1, 1000, 5000);
        CHECK(tl_a.pin_bytes == 5000 + 5000 / 4 + ((size_t)1 << 20) && !tl_b.ws && !tl_b.pin);   // the one growth rule; the other instance untouched
        call(tl_b, -1, 3000, 100);
        CHECK(tl_a.pin != tl_b.pin && tl_a.cur != tl_b.cur && tl_a.ws != tl_b.ws);
        void* pin_a = tl_a.pin; Arena* cur_a = tl_a.cur;
        call(tl_a, id, 1000, 4000);                                                  // the same device named: the same arena, the block not moved
        CHECK(tl_a.pin == pin_a && tl_a.cur == cur_a && tl_a.ws->size() == 1);
        // a slab of 64 MiB holds all of this: warm rounds allocate nothing, whichever instance ran in between
        const size_t slabs_a = tl_a.cur->slabs.size(), slabs_b = tl_b.cur->slabs.size();
        for (int k = 0; k < 3; ++k) { call(tl_b, -1, 3000, 100); call(tl_a, -1, 1000, 5000); }
        CHECK(tl_a.cur->slabs.size() == slabs_a && tl_b.cur->slabs.size() == slabs_b && tl_a.pin == pin_a);
        // growth: a staging need above the block frees it and takes the need, a quarter and 1 MiB; a region above the slab adds one, merged at the next begin
        const size_t big = tl_a.pin_bytes + 1;
        call(tl_a, -1, 1000, big);
        CHECK(tl_a.pin_bytes == big + big / 4 + ((size_t)1 << 20));
        { char* q = NULL; CHECK(tl_b.begin(-1) == STOCS_OK && tl_b.cur->take((size_t)70 << 20, (void**)&q) == STOCS_OK); q[0] = 1; q[((size_t)70 << 20) - 1] = 1; }   // past the first 64 MiB slab
        CHECK(tl_b.cur->slabs.size() == 2);
        call(tl_b, -1, 3000, 100);
        CHECK(tl_b.cur->slabs.size() == 1);
        // a second device: an arena of its own in the same map, the pinned block shared by the instance
        call(tl_a, id + 2, 1000, 100);
        CHECK(tl_a.ws->size() == 2 && tl_a.cur != cur_a && tl_a.dev == id + 2);
        call(tl_a, -1, 1000, 100);
        CHECK(tl_a.cur == cur_a);
        // trim: everything of the instance back, the other instance as it was; twice is harmless
        void* pin_b = tl_b.pin;
        tl_a.trim();
        CHECK(!tl_a.ws && !tl_a.cur && !tl_a.pin && tl_a.pin_bytes == 0 && tl_b.pin == pin_b && tl_b.ws);
        tl_a.trim();
        call(tl_b, -1, 3000, 100);
        tl_b.trim(); tl_b.trim();
        CHECK(!tl_b.ws && !tl_b.pin);
    }
}

int main() {
    const unsigned long long a0 = allocs();
    std::thread t1(worker, 0), t2(worker, 1);
    t1.join(); t2.join();
    CHECK(g_live_dev == 0 && g_live_pin == 0);
    CHECK(allocs() > a0);
    if (g_failed) { fprintf(stderr, "thread_cache_check: %lld checks failed\n", (long long)g_failed); return 1; }
    printf("thread_cache_check: ok, %llu counted allocations, none live\n", allocs() - a0);
    return 0;
}
