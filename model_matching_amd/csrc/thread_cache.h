// thread_cache.h -- the memory that the entry points without a context keep for the calling thread: a grow-only arena per device, so a
// caller that runs one frame after the other does no hipMalloc / hipFree after the first, and one grow-only pinned block for the staging of
// what a call sends up and reads back.  ingest.hip, segment.hip and segment_shapes.hip each keep a thread_local instance of their own
// (three arenas, three pinned blocks: a thread that ingests, segments and takes shapes evicts nothing of any); stocs_trim() gives all back.
#ifndef STOCS_THREAD_CACHE_H
#define STOCS_THREAD_CACHE_H

#include <map>
#include <type_traits>

#include "stocs_ctx.h"

namespace stocs {

// Pointers and sizes only (all zero: nothing held), so that an instance can be thread_local without a destructor: a thread that ends
// without stocs_trim() leaks its cache, as it always did.
struct ThreadCache {
    std::map<int, Arena>* ws;
    Arena* cur;             // the arena of the last begin() ...
    int dev;                // ... and its device
    void* pin;
    size_t pin_bytes;

    // the arena of `device` (< 0: the thread's current one), recycled: the previous call synchronised before it returned
    int begin(int device, Arena** arena = NULL) {
        if (!ws) ws = new std::map<int, Arena>();
        dev = device;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
        cur = &(*ws)[dev];
        if (arena) *arena = cur;
        return cur->reset();
    }
    // the pinned block, holding at least `bytes`: grown by a quarter and 1 MiB past the need, nothing of the old block kept
    int staging(size_t bytes, char** out) {
        if (pin_bytes < bytes) {
            if (pin) { (void)hipHostFree(pin); pin = NULL; pin_bytes = 0; }
            const size_t want = bytes + bytes / 4 + ((size_t)1 << 20);
            STOCS_HIP_CHECK(pinned_malloc(&pin, want));
            pin_bytes = want;
        }
        *out = (char*)pin;
        return STOCS_OK;
    }
    // slabs, map and pinned block back; nothing of the thread's last call may be in flight
    void trim() {
        if (ws) {
            for (std::map<int, Arena>::iterator it = ws->begin(); it != ws->end(); ++it) it->second.destroy();
            delete ws;
            ws = NULL;
            cur = NULL;
        }
        if (pin) { (void)hipHostFree(pin); pin = NULL; pin_bytes = 0; }
    }
};
static_assert(std::is_trivially_destructible<ThreadCache>::value && std::is_trivial<ThreadCache>::value, "ThreadCache must stay a plain struct: it is thread_local");

}  // namespace stocs

#endif
