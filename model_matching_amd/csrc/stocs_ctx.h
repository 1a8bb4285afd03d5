// stocs_ctx.h -- internal state behind the opaque stocs_ctx of include/stocs_hip.h.
#ifndef STOCS_CTX_H
#define STOCS_CTX_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <time.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/stocs_hip.h"
#include "grid_geometry.h"
#include "kdtree.h"
#include "stocs_math.h"
#include "stream_audit.h"

namespace stocs {

void set_error(const char* fmt, ...);

#define STOCS_HIP_CHECK(expr)                                                                  \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            stocs::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return STOCS_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

// Every device allocation of the library goes through here and is counted (stocs_device_alloc_count): a warm context
// must run trial after trial without allocating, and the tests assert exactly that.
extern unsigned long long g_dev_allocs;
inline hipError_t dev_malloc(void** p, size_t bytes) {
    __atomic_fetch_add(&g_dev_allocs, 1ull, __ATOMIC_RELAXED);
    return hipMalloc(p, bytes);
}
template <class T> inline hipError_t dev_malloc(T** p, size_t bytes) { return dev_malloc((void**)p, bytes); }
// pinned host memory goes through the same counter: a hipHostMalloc / hipHostFree inside a trial is as much of a stall
// as a hipMalloc, and stocs_device_alloc_count must see it
inline hipError_t pinned_malloc(void** p, size_t bytes) {
    __atomic_fetch_add(&g_dev_allocs, 1ull, __ATOMIC_RELAXED);
    return hipHostMalloc(p, bytes, hipHostMallocDefault);
}

// Host wall clock of the steps of one entry point, always recorded (a handful of clock reads, no synchronisation of its
// own): when a call takes 80 ms instead of 1, the record says which step it spent them in (stocs_last_call_timing).
struct CallTiming {
    enum { MAX_STEPS = 18 };
    int n;
    const char* label[MAX_STEPS];
    double ms[MAX_STEPS];
    double t_last;
    static double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
    void begin() { n = 0; t_last = now_s(); }
    void lap(const char* what) {
        const double t = now_s();
        if (n < MAX_STEPS) { label[n] = what; ms[n] = (t - t_last) * 1e3; ++n; }
        t_last = t;
    }
};

// Binds the calling thread to the context's device for the duration of an entry point and restores the
// caller's device afterwards (a context may be driven from any thread, one thread at a time).
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// every carved region of a device or pinned block starts on a 256-byte boundary
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Grow-only device block of one owner: grow() leaves it alone when it holds `need` bytes, else waits for the stream (nothing may
// still use the old block), frees it and takes need + need / slack_div.  A caller that has to know whether the block is a new one
// compares `bytes` before and after.
struct DevBlock {
    char* p = NULL; size_t bytes = 0;
    int grow(hipStream_t st, size_t need, size_t slack_div = 4) {
        if (bytes >= need) return STOCS_OK;
        if (p) { STOCS_HIP_CHECK(hipStreamSynchronize(st)); (void)hipFree(p); p = NULL; bytes = 0; }
        const size_t want = need + need / slack_div;
        STOCS_HIP_CHECK(dev_malloc(&p, want));
        bytes = want;
        return STOCS_OK;
    }
    void free() { if (p) (void)hipFree(p); p = NULL; bytes = 0; }
};

// Lays regions out one behind the other, each on a 256-byte boundary: take() gives a region's offset, `total` what the block must
// hold.  Offsets, not pointers: the same layout serves a device block and its mirror in the pinned block (at() on either base).
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t at = total; total += al256(bytes); return at; }
    template <class T> static T* at(void* base, size_t off) { return (T*)((char*)base + off); }
};

// Grow-only device workspace: slabs of plain hipMalloc memory handed out by bumping an offset.  reset() recycles
// everything (nothing of it may still be in flight); a slab that turned out too small is joined by a bigger one
// and the slabs are merged at the next reset, so a steady-state caller never calls hipMalloc / hipFree.
struct Slab { char* p; size_t cap, used; };
struct Arena {
    std::vector<Slab> slabs;
    // nothing that lives in the arena may still be in flight on the device
    int reset() {
        if (slabs.size() > 1) {
            size_t tot = 0;
            for (size_t i = 0; i < slabs.size(); ++i) { tot += slabs[i].cap; (void)hipFree(slabs[i].p); }
            slabs.clear();
            tot += tot;       // slack: trials of one scene differ in size by tens of percent, and 288 GB of HBM make room cheap
            Slab sl = {NULL, tot, 0};
            STOCS_HIP_CHECK(dev_malloc((void**)&sl.p, tot));
            slabs.push_back(sl);
        }
        for (size_t i = 0; i < slabs.size(); ++i) slabs[i].used = 0;
        return STOCS_OK;
    }
    // right after reset(): make sure ONE slab can hold `bytes` (a good estimate up front avoids growing in pieces)
    // headroom 2: a later trial of the same scene with more pair-list entries must not regrow the slab (a 0.6 GB
    // hipFree + hipMalloc inside a trial was the 78 ms outlier of BENCH_r01's pipeline run 4).  A piece of a trial batch is sized
    // against a memory ceiling and asks for little more than it needs; when the device cannot give that either the caller gets
    // STOCS_ERR_NOMEM and cuts the piece (stocs_run_trials).
    int reserve(size_t bytes, double headroom = 2.0) {
        if (slabs.size() == 1 && slabs[0].cap >= bytes) return STOCS_OK;
        destroy();
        Slab sl = {NULL, (size_t)((double)bytes * headroom), 0};
        const hipError_t e = dev_malloc((void**)&sl.p, sl.cap);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); stocs::set_error("arena of %zu bytes: out of device memory", sl.cap); return STOCS_ERR_NOMEM; }
        STOCS_HIP_CHECK(e);
        slabs.push_back(sl);
        return STOCS_OK;
    }
    int take(size_t bytes, void** out) {
        bytes = al256(std::max<size_t>(bytes, 1));
        for (size_t i = 0; i < slabs.size(); ++i)
            if (slabs[i].cap - slabs[i].used >= bytes) { *out = slabs[i].p + slabs[i].used; slabs[i].used += bytes; return STOCS_OK; }
        Slab sl = {NULL, std::max<size_t>(bytes + bytes / 4, slabs.empty() ? ((size_t)64 << 20) : 2 * slabs.back().cap), 0};
        STOCS_HIP_CHECK(dev_malloc((void**)&sl.p, sl.cap));
        sl.used = bytes;
        slabs.push_back(sl);
        *out = sl.p;
        return STOCS_OK;
    }
    void destroy() { for (size_t i = 0; i < slabs.size(); ++i) (void)hipFree(slabs[i].p); slabs.clear(); }
};

// Which grid a build makes (grid.hip).  grid_form (ctx.hip) fills it from the context and the environment switches, once per build; the
// parts that depend on counts known only mid-build are the predicates next to build_grid_gpu, which take the form and the count.
enum GridLayout { GRID_PRUNED, GRID_INDEX_ORDERED, GRID_CENTRE_SORTED };
struct GridForm {
    int div;             // cell edge = epsilon / div, 1 .. 4
    GridLayout layout;   // dominance-pruned lists in index order | every point within r, in index order | ... ordered by distance to the
                         // cell centre, with chunk bounds for the early exit
    int qbits;           // bits of quantised centre distance below the cell in the sort key: 16 centre-sorted, else 0
    int prune_k;         // dominators tried per entry (4, 8, 16); 0 when the lists are not pruned
    bool cones;          // normal cones in the count words (normal_cone.h)
    bool flat;           // asked for: the flat cell table (cell edge epsilon, index order; built if it fits)
    bool octants;        // asked for: octant lines behind long pruned lists (needs the flat table)
    bool own_sort;       // asked for: the library's own sort (sort32.hip) where the incidences are many and the key is short
};

// What one build hands from stage to stage (grid.hip): the geometry, the counts as they become known, and the device arrays in the
// build's workspace (c->grid_ws), where they stay until the next build.
struct GridStages {
    GridBox box;
    size_t n_inc, n_list;           // (cell, point) incidences; padded list entries
    uint32_t n_cells, n_bricks;     // non-empty cells, bricks
    unsigned long long* off;        // per scene point: its first incidence
    uint64_t* keys; uint32_t* vals; // the incidences sorted by key: key, scene point
    const uint32_t* sort_err;       // the own sort's error word, NULL after rocPRIM's
    uint32_t *cflag, *cidx, *bflag, *bidx;   // per incidence: opens a cell / a brick, and the exclusive scans of those flags
    char* scan_tmp; size_t scan_bytes;       // temporary of the 32-bit scans over up to n_inc + 1 words
    uint32_t *cell_first, *cell_brick, *padded, *list_off; uint64_t* cell_key;   // per non-empty cell
    uint32_t *rank, *kept; float* nearest;   // pruned lists: per incidence its place in the stored list (~0: dropped); per cell
    // one zeroed block; its three parts lie 256 bytes apart, as separate workspace takes would, so that the kernels' atomics on them
    // stay apart: [0] longest list; [64..65] kept entries (64 bits); [128..130] long cells, cells with octant lines, entries of those lines
    uint32_t* counters;
    enum { COUNTER_WORDS = 192 };
    uint32_t* longest() const { return counters; }
    unsigned long long* total() const { return (unsigned long long*)(counters + 64); }
    uint32_t* oct() const { return counters + 128; }
};

// Brick grid over the centred scene (replaces the kd-tree of kdtree.h for the restricted-radius
// nearest-neighbour query).  Cell edge h = epsilon.  A cell's candidate list holds every scene
// point whose distance to the cell's box is <= epsilon (+ a 0.1% safety margin), so ONE list scan
// answers the query exactly.  Bricks of 8x8x8 cells exist only where some cell is non-empty.
struct SceneGrid {
    float ox, oy, oz, inv_h;
    int nx, ny, nz;      // cells per axis
    int nbx, nby, nbz;   // bricks per axis
    int n_bricks;
    int64_t n_entries;
    double avg_list_len;   // entries per non-empty cell (of the lists as stored: after the dominance pruning, when it is on)
    double avg_dilated_len;   // ... of every scene point within r of the cell box (what the list held before pruning)
    bool pruned;           // the lists hold only points that can be the nearest neighbour of some position in their cell (grid.hip)
    // what the last build did, for stocs_get_grid_info (records only: nothing reads them back into a decision)
    int div;               // cell edge = epsilon / div
    int sort_kind;         // STOCS_GRID_SORT_*: which sort ordered the incidences (0: none ran)
    int prune_group, prune_k;   // lanes per cell and dominators per entry of the prune kernel; 0, 0 when the lists are not pruned
    int64_t n_inc;         // (cell, point) incidences
    int64_t n_cells;       // non-empty cells
    int longest_list;      // entries of the longest stored list (before padding)
    // octant lines (octant_lists.h): cells whose stored list is longer than a line, those of them whose flat-table word names an octant
    // block, and the entries of their octant lines before padding; all 0 on a grid without them.  n_entries counts the plain lists only
    int64_t n_long_cells, n_octant_cells, n_octant_entries;
    // the lines are written by build_octant_lines once the scene's scoring work makes them pay (lcp.hip); until then `stages` keeps what
    // that call needs of the build (its temporaries stay in the build's workspace until the next build)
    bool oct_pending;
    GridStages stages;
    int32_t* d_top;     // nbx*nby*nbz -> brick id or -1
    uint4* d_flat;       // the same cell words addressed directly, (cz*ny + cy)*nx + cx, when the box is small enough (sparse
                         // scenes, cell edge eps): saves the LCP kernel the dependent `top` look-up; else NULL
    uint4* d_cells;      // n_bricks*512: (offset, count, sub-cell mask lo, hi); mask bit s set <=> some scene
                         // point lies within epsilon of sub-cell s (4x4x4 sub-cells, x fastest)
    float4* d_list;      // (x, y, z, bits(scene index))
    float* d_chunk_r;    // dense scenes only: lists sorted by distance from the cell centre; per 8-entry chunk a
                         // lower bound of that distance (early exit by the triangle inequality); else NULL
    float h;             // cell edge
    bool has_cones;      // the count word of a cell carries a cone of its list's scene normals above the 16-bit list length (normal_cone.h);
                         // false (empty scene, STOCS_GRID_CONES=0): those bits are zero and no gated kernel form runs
    bool has_nearest;    // dense grids with cell edges below epsilon: the z word of a cell is a lower bound of the distance from the
                         // cell centre to the nearest listed point (the sub-cell mask it replaces is all ones there)
    // Distance field of the scene on a coarse grid (cell edge cg_g >= epsilon), for the patch test of the scan kernels (lcp.hip):
    // d_dist[cell] = distance from the cell's centre to the nearest scene point, rounded down, capped at cg_cap.  The box covers the
    // scene's bounding box widened by cg_cap + cg_g on every side, so a position outside it is at least cg_cap from every scene point.
    // The memory is taken with the grid (no allocation later); the values are filled on first use (fill_cull_field).
    float* d_dist;
    bool dist_ready;
    // Normal cones over the same cells (patch_normals.h), for models the shared-list forms score: d_ncone lies right behind d_dist in
    // one block of cg cells each (a kernel finds it from d_dist and the cell counts), one 32-bit cone per cell of the normals of every
    // scene point within pn_rb of the cell's centre; d_nsum: the build's fixed-point axis sums, three words per cell.  Filled with
    // d_dist (fill_cull_field); NULL: no cone field.  pn_reach: what a kernel may rely on (pn_reach_for_kernel); pn_w: cells a point reaches
    uint32_t* d_ncone;
    int32_t* d_nsum;
    bool ncone_ready;
    float pn_rb, pn_reach;
    int pn_w;
    float cg_ox, cg_oy, cg_oz, cg_g, cg_inv_g, cg_cap;
    int cg_nx, cg_ny, cg_nz, cg_w;   // cg_w: cells a point reaches on either side (ceil(cap / g))
    double bb_mn[3], bb_mx[3];       // bounding box of the centred scene
};
// No grid: every pointer NULL, every count and record zero.  The memory is the arenas' (c->grid_mem, c->grid_ws), which the next build resets
inline void reset_grid(SceneGrid& g) { g = SceneGrid(); }

// Model PPF index on the device: every ordered pair stored once under its own quantised key F
// (CSR over the dense key space), plus the dilated existence bitmap ("is K a key of the
// reference's 128-fold map?").
struct PpfIndex {
    bool built;
    int tr, rot, NA, nD;          // angle bins NA = 180/rot + 1, distance bins nD
    int64_t n_keys;               // nD*NA^3
    int64_t n_pairs;
    uint32_t* d_bucket_start;     // n_keys + 1
    uint32_t* d_pairs;            // n_pairs: (id1 << 16) | id2, sorted inside each bucket
    uint32_t* d_exists;           // bitmap over the key space, n_keys bits
    std::vector<uint32_t> h_bucket_start;  // host copy (planning of the lookups)
    std::vector<uint32_t> h_exists;        // host copy of the bitmap (single-key query API)
    int64_t n_nonempty_buckets, n_exist_keys;
};

struct BaseRec {
    int ids[4];
    float inv1, inv2;
};

// rows 6-7 on the device: ordered base + invariants of one attempt (try_sampled_base, stocs.cpp:224-268)
struct BaseOut { int32_t ids[4]; float inv[2]; int32_t valid; int32_t pad; };

struct Candidate {
    float T[16];     // centred frames (scored), stocs.cpp:923
    float pose[16];  // camera frame (returned), stocs.cpp:925-937
    float lcp;
    int base_index;
};

// The two records that pass between the candidate phase (transform.hip) and the congruent state that resolves them (congruent.hip)
struct XformJob { int32_t s[4]; int32_t q[4]; };                // scene base ids, model quad ids
// quad `rank` of `base` -> job `dst`; sorted: rank counts in the base's materialised, sorted run (else in its walk order).  Aligned so that
// the kernels read and write a pick as one 128-bit access
struct alignas(16) Pick { int32_t base, rank, dst, sorted; };
// stocs_match_one_object.cpp:126: a base with STRICTLY fewer quads than the per-base maximum is used whole, in the std::set order of
// stocs.cpp:860-866 (materialised and sorted); one at the maximum or above it contributes a seeded draw of max_per_base quads
STOCS_HD bool base_used_whole(long long nq, int max_per_base) { return nq < max_per_base; }
STOCS_HD long long base_pick_count(long long nq, int max_per_base) { return base_used_whole(nq, max_per_base) ? nq : (long long)max_per_base; }

struct Thresholds {
    float lcp_dot_lo;   // normal test true  <=>  lcp_dot_lo <= dot <= 1
    float ang_dot_hi;   // internal-angle reject <=> (ang_dot_hi <= dot <= 1) || (-1 <= dot <= ang_dot_lo)
    float ang_dot_lo;
};

// The records of stocs_ctx::timing: the last call of each of these entry points.  stocs_last_call_timing serves the slots below
// TIMING_VSD_MESH, stocs_mesh_last_call_timing that one
enum TimingSlot {
    TIMING_CONGRUENT,        // stocs_find_congruent_all
    TIMING_TRANSFORMS,       // stocs_make_transforms
    TIMING_VERIFY,           // stocs_verify_all
    TIMING_TRIALS,           // stocs_run_trials
    TIMING_POSE_ERRORS,      // stocs_pose_errors
    TIMING_POSE_ERRORS_SYM,  // stocs_pose_errors_sym
    TIMING_SYMMETRY,         // stocs_symmetry_errors
    TIMING_VSD,              // stocs_pose_errors_vsd
    TIMING_VSD_MESH,         // stocs_pose_errors_vsd_mesh
    TIMING_COUNT
};

// Per-feature state of a context (stocs_ctx::state): a struct that its owner file defines, made at the feature's first call
// (ctx_state) and deleted by stocs_ctx_destroy in the order of this enum.  The struct names its slot (`static const StateOwner OWNER`)
// and frees its device blocks in its destructor.  A new feature adds an enumerator here and a struct in its own file, nothing else
enum StateOwner {
    OWN_REFINE,          // refine.hip: the model's correspondence grid of stocs_refine_poses and its grow-only workspace
    OWN_TRACK,           // track.hip: stocs_track_poses's grow-only workspace and the details of its last call
    OWN_DEPTH,           // depth_frame.h: the frame of stocs_ctx_set_frame and stocs_depth_check_poses's grow-only workspace
    OWN_INSTANCES,       // instances.hip: stocs_select_instances's grow-only workspace
    OWN_RENDER,          // render.hip: the grow-only workspace of stocs_render_poses and its kin
    OWN_SCENE,           // scene.hip: the grow-only workspaces of stocs_scene_footprints and stocs_scene_select
    OWN_POSE_ERROR,      // pose_error.hip: the grow-only workspace of stocs_pose_errors and its kin, the cached diameter
    OWN_POSE_ERROR_SYM,  // pose_error_sym.hip: the grow-only workspace of stocs_pose_errors_sym and its detail form
    OWN_SYMMETRY,        // symmetry.hip: the model's self-distance grid of stocs_symmetry_errors and its grow-only workspace
    OWN_VSD,             // vsd.hip: the grow-only workspace of stocs_pose_errors_vsd and stocs_render_depth
    OWN_MESH,            // mesh.hip: the triangle mesh of stocs_ctx_set_mesh on the device
    OWN_RENDER_MESH,     // render_mesh.hip: the grow-only workspaces of stocs_render_poses_mesh and its kin
    OWN_REFINE_VISIBLE,  // refine_visible.hip: the grow-only workspace of stocs_refine_poses_visible and its detail form
    OWN_COUNT
};
struct StateSlot { void* p = NULL; void (*del)(void*) = NULL; };

}  // namespace stocs

struct stocs_ctx {
    stocs_params prm;
    int device;
    hipStream_t stream;       // the stream all work is issued on
    hipStream_t own_stream;   // created with the context; `stream` may point to a caller's stream instead
    hipStream_t aux_stream;   // second stream of the context for work that is independent of `stream` until an event joins it
    hipEvent_t ev0, ev1, ev_fork, ev_join;
    hipEvent_t ev_t[10];   // stocs_find_congruent_all: clock stamps around its device groups (opt-in) and three ordering events, named by CongEvent below; other calls borrow slots as plain clock stamps
    int nS, nM;
    stocs::Thresholds thr;

    // host copies (centred unless stated)
    std::vector<stocs::V3> h_spos, h_snrm, h_mpos, h_mnrm, h_mpos_raw, h_munit;
    std::vector<float> h_sprob;       // class_probability_ (decays in instance mode)
    std::vector<float> h_sprob0;      // class probabilities as given at construction (stocs_reset_trial)
    std::vector<int32_t> h_spix;      // row, col
    stocs::V3 centroid_scene, centroid_model, gcenter;
    float ratio;
    std::vector<int32_t> h_mperm;     // patch order of the model used by the LCP kernel (sorted slot -> model index)

    // device clouds
    char* d_scene_mem; size_t scene_cap;   // one grow-only slab for the three scene arrays below (a new frame reuses it)
    float4* d_spos;    // xyz + class prob
    float4* d_snrmw;   // unit normal + class prob weight (what LCP adds, stocs.cpp:1033)
    int2* d_spix;
    float4* d_mpos;    // centred model, original order (xyz, 0)
    float4* d_mnrm;
    float4* d_munit;   // unit-cube model (pairCreationFunctor.h:96-132)
    float4* d_mpos_raw;  // un-shifted model positions (index build)
    float4* d_mpos_s;  // copies in patch order for the LCP kernel (positions NaN-padded to whole 64-point steps + one; w = the packed model normal, normal_cone.h)
    float4* d_mnrm_s;
    int32_t* d_mperm;
    float4* d_mpatch;  // per 64-point step of the sorted model: bounding sphere (centre xyz, radius) of its points (patch test, lcp.hip)
    float4* d_msub;    // per 16-point sub-patch (four per step, NaN spheres behind the model): the unit of the patch test at lcp_cull_unit = 16
    float patch_r_ref; // the radius most patches stay below (sizes the cap of the scene's distance field)
    float sub_r_ref;   // ... most 16-point sub-patches stay below (sizes the reach of the scene's cone field, patch_normals.h)
    int lcp_cull;      // 1: the scan kernels skip the 64-point steps whose bounding sphere is farther than epsilon from every scene point
    int lcp_cull_unit; // points per sphere of that test: 16 (default; live sub-patches are packed four to a step) or 64 (whole steps)
    double lcp_cull_after;   // lcp_cull == 1: the distance field is filled once this many point queries were scored against the scene (default 1e9)
    bool prev_scene_warm;    // the scene before this one crossed that threshold: a stream of frames will again, so the field of a new frame
                             // is filled right away, on the auxiliary stream (cull_pending: the scoring stream has not waited for it yet)
    bool cull_pending;
    hipEvent_t ev_cull;
    int scene_scored;  // scoring launches against the current scene
    double scene_work; // candidates x model points scored against the current scene so far (the distance field is filled when it pays)

    stocs::SceneGrid grid;
    stocs::Arena grid_mem;   // top / cells / list / chunk_r of the current grid (reset by every build)
    stocs::Arena grid_ws;    // temporaries of a grid build
    int grid_div;   // cell edge = epsilon / grid_div
    int grid_prune; // 1 (default): the grid's lists are dominance-pruned (grid.hip); 0: the layouts of rounds 2-4 (STOCS_GRID_PRUNE, read at stocs_ctx_create)
    int lcp_variant;   // -1: automatic; else stocs_set_option("lcp_variant")
    int device_clock;  // 1: stocs_find_congruent_all records HIP events between its kernel groups ("device: ..." steps of stocs_last_call_timing); default 0 (STOCS_DEVICE_CLOCK=1 turns it on)
    int lcp_split;     // 1: four wavefronts share one candidate (default), 0: one wavefront per candidate
    int lcp_flat;      // 1: build and use the flat cell table when it fits (default), 0: brick look-ups only
    unsigned long long pn_launches;   // scoring launches so far that ran a shared-list form with the cone test on (stocs_patch_normal_info)
    int lcp_patch_normals; // 1 (default): the shared-list forms' patch test also rules sub-patches out by normal cones (patch_normals.h; same scores)
    int lcp_normal_gate;   // 1 (default): the queue kernel drops queries whose cell's normal cone cannot pass the normal test (same scores)
    int lcp_order;     // 0: candidates in batch order; 1: spatially ordered processing of big batches; 2: + XCD-contiguous blocks
    stocs::DevBlock order;   // keys / permutation / sort scratch of the ordering
    // "exact_ties" (stocs_set_option): tied nearest-neighbour queries answered by the reference-order kd-tree (kdtree.h).  The tree
    // of the current scene is built at the first exact-mode scoring call after a scene change (at stocs_ctx_set_scene when the
    // option is already on) and lives in one grow-only device block: tie counters (flagged, changed) | nodes | points in tree order
    int exact_ties;
    bool kd_ready;                 // kd_host / d_kd hold the tree of the current scene
    stocs::KdTreeHost kd_host;
    stocs::DevBlock kd;
    const stocs::KdNodeP* d_kd_nodes;
    const float4* d_kd_pts;
    unsigned long long* d_ties;    // [0] tied queries seen, [1] those whose reference answer differs from the largest-index rule
    bool ties_started;             // the current entry point has zeroed the counters (stocs_last_tie_counts reads 0 / 0 otherwise)
    // class-mode sampling, lean kernel (sample.hip): exclusive prefix sums of the prior's 2^32 fixed-point weights in scene order (S + 1
    // entries), recomputed when the class probabilities on the device have changed (prior_epoch) or the scene has (cdf_n)
    stocs::DevBlock cdf; size_t cdf_n; unsigned long long prior_epoch, cdf_epoch;
    stocs::PpfIndex index;

    // image-space state of instance mode (stocs.hpp:153-155)
    bool has_edge;
    std::vector<uint8_t> edge_map;   // png values (all zero = "file absent", stocs.cpp:117-119)
    void* inst;                      // device-side state of instance mode (sample.hip, InstanceState): runs of the edge map,
                                     // previous_segment / segmentation_buffer / seg_mask_<n> per scene point, the decaying prior

    std::vector<int32_t> last_segment;   // `segment` of the last instance-mode attempt (stocs.cpp:628-638)

    // run state
    std::vector<stocs::BaseRec> bases;
    // a batch of independent trials in one set of launches (stocs_run_trials, trials.hip): `bases` is then the concatenation of the
    // trials' base sets, and these say whose each base is.  All empty outside such a batch (one trial, the calls' own seed).
    std::vector<uint64_t> base_seed;        // per base: seed of its trial
    std::vector<int32_t> base_local;        // per base: its slot in its own trial's base set
    std::vector<int32_t> trial_first_base;  // per trial of the batch (+ 1): first base
    std::vector<int32_t> trial_cand_off;    // per trial of the batch (+ 1): first candidate (filled by stocs_make_transforms)
    const float4* snrmw_trial0;             // instance-mode batches: trial t scores against the weights at snrmw_trial0 + t * snrmw_stride bytes
    size_t snrmw_stride;
    const int32_t* lcp_cand_trial;          // != NULL (with snrmw_override = trial 0's copy): candidate i of the launch scores against trial lcp_cand_trial[i]'s copy
    const float4* snrmw_override;           // != NULL: the scoring kernel reads its scene normals + weights here (one trial of such a batch)
    void* trials;                           // results of the last stocs_run_trials (trials.hip, TrialBatch)
    // congruent quads: only their per-base counts live here (quad_off[b+1] - quad_off[b]); `cong` (congruent.hip,
    // CongruentState) keeps what is needed to produce the quads of a base on demand, packed with quad_id_bits
    // bits per model id below the base id
    void* cong;
    std::vector<unsigned long long> quad_off;
    int quad_id_bits;
    // candidates of the last stocs_make_transforms: device-resident (compacted, in pick order) as
    // T[n][16] | pose[n][16] | lcp[n] | base[n] inside d_cand; `cands` is the host mirror, filled on demand
    std::vector<stocs::Candidate> cands;
    char* d_cand;
    size_t cand_bytes;
    int n_cands, cand_cap;
    bool cands_stale;   // the device copy is newer than `cands`
    float best_lcp;
    int best_index;

    unsigned long long* d_best;   // 8-byte arg-max key
    bool best_is_zero;            // *d_best was zeroed on the stream by the last stocs_make_transforms and not used since

    // pinned host block for the small device-to-host read-backs of the entry points (totals, offsets, keys): a copy into
    // pageable memory goes through the runtime's own staging and is one more thing that can stall (ensure_pinned grows it)
    void* h_pin;
    size_t pin_bytes;
    stocs::CallTiming timing[stocs::TIMING_COUNT];

    stocs::StreamAudit audit;   // STOCS_DEBUG_STREAMS=1: happens-before check of the two-stream sections (stream_audit.h); off otherwise

    // scratch
    void* d_scratch;
    size_t scratch_bytes;

    // what the last stocs_sample_bases / stocs_run_trials* call ran, class or instance mode (sample.hip; read by stocs_last_sampling_form): host
    // bookkeeping only.  kernel < 0: no class-mode call yet
    struct { int kernel, threads; size_t lds; int cap, launches, redone; } last_form;

    stocs::StateSlot state[stocs::OWN_COUNT];   // per-feature state, see StateOwner
};

namespace stocs {
// the state of T's feature on the context, made at first use / as it stands, NULL when the feature has not run (for the readers)
template <class T> inline T* ctx_state(stocs_ctx* c) {
    StateSlot& s = c->state[T::OWNER];
    if (!s.p) { s.p = new T(); s.del = [](void* p) { delete (T*)p; }; }
    return (T*)s.p;
}
template <class T> inline T* ctx_state_if(const stocs_ctx* c) { return (T*)c->state[T::OWNER].p; }
inline void clear_candidates(stocs_ctx* c) { c->cands.clear(); c->n_cands = 0; c->cands_stale = false; }
// the base set is (again) one trial's: whoever replaces or extends it outside stocs_run_trials calls this first
inline void clear_trial_batch(stocs_ctx* c) {
    if (c->base_seed.empty() && c->trial_first_base.empty()) return;
    c->base_seed.clear(); c->base_local.clear(); c->trial_first_base.clear(); c->trial_cand_off.clear();
    c->snrmw_trial0 = NULL; c->snrmw_stride = 0;
    c->bases.clear(); c->quad_off.clear(); clear_candidates(c);   // what is left of the batch's last piece means nothing to a single trial
}
// The ev_t slots as stocs_find_congruent_all uses them.  The first seven are CLOCK STAMPS only: recorded when the device clock is on
// (c->device_clock; an event between two kernels costs ~5 us on this runtime) and read after the call's closing synchronisation.
// The last three also ORDER work: the host waits on EV_SURVIVORS_READ in every reduced pass, and EV_Q_MARKED / EV_P_MARKED are the
// cross edges of the two-stream form (each list's counts test the OTHER list's occupancy); those two are recorded when the pass has
// two streams or the device clock is on.
enum CongEvent {
    EV_SORT_BEGIN = 0, EV_Q_SORTED = 1, EV_P_SORTED = 2, EV_SIDES_JOINED = 3, EV_JOIN_COUNTED = 4, EV_PASS_END = 5, EV_REDUCE_BEGIN = 6,
    EV_SURVIVORS_READ = 7, EV_Q_MARKED = 8, EV_P_MARKED = 9
};
// An event edge between the context's two streams and its mirror in the stream audit, as one call: `record` stamps what `from` holds
// now, `wait` puts whatever `to` is given from now on behind it.  Streams by their audit index: 0 = c->stream, 1 = c->aux_stream.
inline hipStream_t ctx_stream(const stocs_ctx* c, int s) { return s ? c->aux_stream : c->stream; }
inline int stream_edge_record(stocs_ctx* c, hipEvent_t ev, int from) {
    STOCS_HIP_CHECK(hipEventRecord(ev, ctx_stream(c, from)));
    c->audit.record(ev, from);
    return STOCS_OK;
}
inline int stream_edge_wait(stocs_ctx* c, hipEvent_t ev, int to) {
    STOCS_HIP_CHECK(hipStreamWaitEvent(ctx_stream(c, to), ev, 0));
    c->audit.wait(to, ev);
    return STOCS_OK;
}
inline int stream_edge(stocs_ctx* c, hipEvent_t ev, int from, int to) {
    const int rc = stream_edge_record(c, ev, from);
    return rc ? rc : stream_edge_wait(c, ev, to);
}
inline float* cand_T(stocs_ctx* c) { return (float*)c->d_cand; }
inline float* cand_P(stocs_ctx* c) { return (float*)c->d_cand + (size_t)c->cand_cap * 16; }
inline float* cand_lcp(stocs_ctx* c) { return (float*)c->d_cand + (size_t)c->cand_cap * 32; }
inline int32_t* cand_base(stocs_ctx* c) { return (int32_t*)((float*)c->d_cand + (size_t)c->cand_cap * 33); }
int ensure_scratch(stocs_ctx* c, size_t bytes);
int ensure_pinned(stocs_ctx* c, size_t bytes);   // c->h_pin of at least `bytes` (nothing may still be copying into the old block)
enum { PIN_CONGRUENT = 0, PIN_TRANSFORMS = 256, PIN_VERIFY = 512, PIN_BEST = 768, PIN_GRID = 1024, PIN_VAR = 1280 };   // fixed slots, then the per-call variable part
struct PinGrid {   // PIN_GRID: the read-backs of a grid build and of build_octant_lines (grid.hip)
    unsigned long long n_inc, n_kept;      // incidences, entries kept by the pruning
    uint32_t n_cells, n_bricks, sort_err;  // non-empty cells, bricks, the own sort's error word
    uint32_t n_list, longest;              // padded list entries, entries of the longest stored list
    uint32_t n_long_cells, n_octant_cells, n_octant_entries;   // (the last two are one 8-byte copy)
};
static_assert(sizeof(PinGrid) <= PIN_VAR - PIN_GRID, "PinGrid outgrew its pinned slot");
// The per-call staging: *h = the variable part of the pinned block, holding at least `bytes`.  The one place where the block grows under a
// call: the stream is synchronised first if it has to move (nothing may still be copying into the old block).
int pinned_var(stocs_ctx* c, size_t bytes, char** h);
// ... split into what the call sends up (in_bytes at *h_in) and, behind it at al256(in_bytes), the mirror of its read-back (back_bytes)
int pinned_for(stocs_ctx* c, size_t in_bytes, size_t back_bytes, char** h_in, char** h_back);
// d_best8 != NULL: the kernel's epilogue also takes the arg-max of compute_best_transform over the batch into that word (zeroed in front)
int launch_lcp(stocs_ctx* c, const float* d_T16, int n, float* d_lcp, int32_t* d_hit, uint8_t* d_counted, unsigned long long* d_best8, uint32_t id_offset);
// every scoring entry point calls this first: the tie counters of stocs_last_tie_counts then cover that call alone (no device work)
inline void begin_scoring_call(stocs_ctx* c) { c->ties_started = false; }
// refine.hip: the point-to-plane refinement as a step on device-resident hypotheses (stocs_refine_poses[_robust], the trial batches'
// post-processing, the tracker).  One settings value covers both forms: plain is keep_ratio 1 with the gate off (refine_plain).
struct RefineSettings { int iterations; float distance, keep_ratio, min_normal_cos; };   // min_normal_cos below -1: gate off
inline RefineSettings refine_plain(int iterations, float distance) { return RefineSettings{iterations, distance, 1.0f, -2.0f}; }
inline const char* robust_setting_error(float keep_ratio, float min_normal_cos) {
    if (!(keep_ratio > 0.0f && keep_ratio <= 1.0f)) return "keep_ratio must be in (0, 1]";
    if (!(min_normal_cos <= 1.0f)) return "min_normal_cos must be <= 1 (below -1: gate off)";
    return NULL;
}
struct RefineWork {   // what refine_prepare planned (value-initialised: nothing)
    RefineSettings s = {};
    void* d_hyp = NULL; float* d_Tin = NULL; int32_t* d_idx = NULL; double* d_part = NULL;   // d_Tin: the n centred T16 to refine; d_idx: nsrc source indices
    float* d_Tout = NULL; float* d_Pout = NULL; float* d_lcp = NULL; int32_t* d_nc = NULL; int32_t* d_it = NULL;   // contiguous outputs, out_bytes in all
    size_t out_bytes = 0;
    int n = 0, nsrc = 0, nchunks = 0;
    // rows (keep_ratio < 1): rank words | model indices of `group` hypotheses x nsrc and their select results, shared by the groups of
    // consecutive hypotheses the n are refined in; else one group of n and no rows
    bool rows = false; int group = 0;
    uint32_t* d_word = NULL; int32_t* d_match = NULL; void* d_sel = NULL;
};
enum { REFINE_ONE_GROUP = 1, REFINE_ROWS = 2 };   // refine_prepare: never group (the caller bounds n x nsrc itself); rows even at keep_ratio 1
// The model grid for s.distance, the workspace of n hypotheses over nsrc source points and, with rows, the group size and the rows
// (all grow-only; may synchronise when one has to be built or grown: nothing of them may be in flight).  who: the entry point, for messages
int refine_prepare(stocs_ctx* c, const char* who, int n, int nsrc, const RefineSettings& s, int flags, RefineWork* w);
// init (d_live != NULL: hypothesis k takes part only when d_live[k]), group by group s.iterations x (evaluate, solve), final, the LCP
// launch over all n -- on the stream, no copy, no synchronisation.  Input: w.d_Tin; the source is w.d_idx[0 .. nsrc) when use_idx, else
// every scene point.  w.d_nc: the pairs that counted in the last evaluated iteration.  *n_groups (may be NULL): the groups it ran
int refine_enqueue(stocs_ctx* c, const RefineWork& w, bool use_idx, const int32_t* d_live, int* n_groups);
// cluster.hip: greedy_clustering of every trial of a batch piece on the device (see there); no synchronisation
struct TrialClusterArgs { float fraction; int32_t count; float min_distance, min_angle; float sym[3]; };
// hypothesis slots of a trial with n candidates: the reference's `size() > count` break keeps up to count + 1 of them.  The one rule
// for stocs_run_trials_post and stocs_cluster_trials_device (the kernel's `cap`)
inline int32_t trial_hyp_slots(int count, long long n) { const long long m = (long long)count + 1; return (int32_t)(m < n ? m : n); }
int enqueue_trial_cluster(stocs_ctx* c, int n_trials, const float* d_P, const float* d_lcp, const int32_t* d_cand_off, const float* d_best18,
                          const TrialClusterArgs& a, uint8_t* d_alive, const int32_t* d_hyp_off, int32_t* d_hyp_cnt, int32_t* d_hyp_idx);
int ensure_kdtree(stocs_ctx* c);   // kdtree.hip: the kd-tree of the current scene on the device (exact_ties); synchronises
int sample_trials(stocs_ctx* c, int mode, int nT, const uint64_t* seeds, int nA, float dispersion, BaseOut* res_host, const float4** snrmw0, size_t* snrmw_stride);   // sample.hip
int build_ppf_index(stocs_ctx* c);
int build_grid_gpu(stocs_ctx* c, const GridForm& form);   // c->grid from c->d_spos (device) and c->h_spos (bounding box only)
int prepare_cull_field(stocs_ctx* c);   // geometry + memory of SceneGrid::d_dist for the current grid and model (end of a grid build)
int build_octant_lines(stocs_ctx* c);                          // the octant lines of the current grid, on c->stream, once per scene (grid.hip)
int fill_cull_field(stocs_ctx* c, hipStream_t st = NULL, bool cones = true);   // the values, on st (NULL: c->stream); no synchronisation.  cones: also
                                                                               // the cone field, when the grid has one, it is not yet filled and lcp_patch_normals is on
// congruent.hip, the device side of stocs_make_transforms: the bases used whole materialised and sorted, then picks -> jobs (see there)
extern "C" int stocs_internal_prepare_small(stocs_ctx* c, int max_per_base);
extern "C" int stocs_internal_make_jobs(stocs_ctx* c, const Pick* picks_host, const Pick* picks_dev, int n, XformJob* d_jobs_out, const unsigned int** d_unresolved_out);
extern "C" void stocs_internal_free_congruent(stocs_ctx* c);
extern "C" void stocs_internal_invalidate_congruent(stocs_ctx* c);
extern "C" void stocs_internal_free_instance(stocs_ctx* c);
extern "C" void stocs_internal_free_trials(stocs_ctx* c);
// the congruent phase with a ceiling on its device memory: *too_big != 0 (and STOCS_OK) when the pair lists of the context's base set
// would need more than max_bytes (0: no ceiling) or exceed 2^32 entries -- a trial batch then splits the base set and tries again
extern "C" int stocs_internal_find_congruent(stocs_ctx* c, int64_t* total_quads, size_t max_bytes, int* too_big);
extern "C" void stocs_internal_invalidate_instance(stocs_ctx* c);
int plan_lookup(const PpfIndex& ix, const int* K, std::vector<std::pair<uint32_t, uint32_t> >* ranges);
void compute_thresholds(const stocs_params& prm, Thresholds* t);
}  // namespace stocs

#endif
