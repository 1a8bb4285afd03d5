// octant_lists.h -- per-octant lines of a long cell's candidate list (grid.hip builds them, the FLAT forms of lcp_coopq_kernel read them).
// Shared by host and device; compiles as plain C++ (tests/cpp/octant_lists_check.cpp runs it on the host against a brute-force scan).
//
// The dominance pruning of grid.hip works over the whole cell box, and a cell the surface crosses keeps every point that is nearest
// SOMEWHERE in it: 9-14 points at 1.6-2 mm sampling and 5 mm cells, two 128-byte lines.  The query already knows which octant of the cell it
// is in (bit 1 of its quarter-cell coordinates), and over an octant box far fewer points survive.  A cell whose stored list is longer
// than one line therefore gets a block of eight lines of 8 entries behind its list, one per octant, and -- when every octant fits its
// line -- a flagged word in the flat cell table: x = (offset of the block) | 0x80000000, and 8 for the count in y.  The kernel then reads
// the line at (x & 0x7FFFFFFF) + octant_line_start(sub-cell) as a list of 8 entries.  The plain list, the brick-table word, the cone and
// the sub-cell mask stay what they were; every reader but the FLAT forms never sees the flag.
//
// Exactness (the same point, the same index, the same tie rule as the cell's plain list):
//   * the kernel puts a query in an octant by the float floor that puts it in its cell (floor((q - o) * 4 / h) >> 1 & 1 per axis), so the
//     query lies inside the octant box widened by the slack the cell box is widened by (`hw` below = h / 4 + that slack);
//   * the winner W of the plain list is within epsilon of the query, hence within r of the octant box (r carries the same rounding
//     allowance as for the cell box): W passes the range test;
//   * an octant line is built from the cell's STORED list, so it is a subset of it and the cell's normal cone covers it; W is in the stored
//     list (it is never dominated over the cell);
//   * W is not dominated over the octant: a dominator is an entry of the stored list whose float distance is strictly smaller at every
//     position of the widened octant box (the margin covers the float evaluation of both squared distances) -- it would have beaten W
//     in the plain list;
//   * the line keeps the ascending index order, padded with copies of its last entry (an equal distance at the same index changes
//     nothing under `<=`): the winner over a subset that contains the winner over the whole list is that same entry.
#ifndef STOCS_OCTANT_LISTS_H
#define STOCS_OCTANT_LISTS_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STOCS_OCT_HD __host__ __device__ __forceinline__
#else
#define STOCS_OCT_HD inline
#endif

namespace stocs {

#define STOCS_OCTANT_FLAG 0x80000000u
#define STOCS_OCTANT_LINE 8u          // entries of an octant's line: one 128-byte line of 16-byte entries
#define STOCS_OCTANT_BLOCK 64u        // entries reserved behind the plain list of a long cell: eight lines
#define STOCS_OCTANT_K 8              // dominators tried per entry

// the x word of a flat-table cell: a list offset (below 2^31), or the offset of an octant block with the flag above it
STOCS_OCT_HD uint32_t octant_word_pack(uint32_t block_off) { return block_off | STOCS_OCTANT_FLAG; }
STOCS_OCT_HD bool octant_word_flagged(uint32_t x) { return (x & STOCS_OCTANT_FLAG) != 0u; }
STOCS_OCT_HD uint32_t octant_word_offset(uint32_t x) { return x & ~STOCS_OCTANT_FLAG; }

// octant of a position from its quarter-cell coordinates (c4 = floor((q - o) * 4 / h) per axis; c4 & 3 is the sub-cell): x fastest
STOCS_OCT_HD uint32_t octant_of_quarter(int c4x, int c4y, int c4z) {
    return (uint32_t)(((c4x >> 1) & 1) | (((c4y >> 1) & 1) << 1) | (((c4z >> 1) & 1) << 2));
}
// ... and of sub-cell s = (sz << 4) | (sy << 2) | sx of the cell's 64-bit mask, which the kernel has at hand
STOCS_OCT_HD uint32_t octant_of_subcell(uint32_t s) { return ((s >> 1) & 1u) | (((s >> 3) & 1u) << 1) | (((s >> 5) & 1u) << 2); }
// Where an octant's line starts inside the block, from a sub-cell of that octant: the octant is bits 1, 3 and 5 of s, and
// v + 8 v of v = s & 0x2A has them at bits 4, 3 and 5 (its other set bits are 1, 6 and 8: no two meet, no carry).  Three instructions
// in the kernel's step where the octant number takes six; the lines of a block are therefore in the order y, x, z -- a fixed
// permutation of the octants, the same for the builder and the reader.
STOCS_OCT_HD uint32_t octant_line_start(uint32_t s) { const uint32_t v = s & 0x2Au; return ((v << 3) + v) & 0x38u; }
STOCS_OCT_HD uint32_t octant_line_start_of_octant(uint32_t o) { return octant_line_start(((o & 1u) << 1) | (((o >> 1) & 1u) << 3) | (((o >> 2) & 1u) << 5)); }
STOCS_OCT_HD uint32_t octant_line_offset(uint32_t x, uint32_t s) { return octant_word_offset(x) + octant_line_start(s); }

// The dominance predicate of grid.hip, in double.  u = p - centre, u' = p' - centre; n2 = |u|^2, dn2 = |u'|^2, l1 = |u - u'|_1.  The
// difference of the squared distances from a position centre + s is |u|^2 - |u'|^2 - 2 s . (u - u'), so its minimum over the box
// |s_k| <= hw is n2 - dn2 - 2 hw l1: above the margin, p' is strictly nearer than p at every position of the box, float evaluation included.
STOCS_OCT_HD bool dominated_over_box(double n2, double dn2, double l1, double hw, double margin) {
    return (n2 - dn2) - 2.0 * hw * l1 > margin;
}

// squared distance from p to the box centre +- hb per axis (0 inside)
STOCS_OCT_HD double octant_box_dist2(double px, double py, double pz, const double ctr[3], double hb) {
    const double ax = fabs(px - ctr[0]) - hb, ay = fabs(py - ctr[1]) - hb, az = fabs(pz - ctr[2]) - hb;
    const double dx = ax > 0.0 ? ax : 0.0, dy = ay > 0.0 ? ay : 0.0, dz = az > 0.0 ? az : 0.0;
    return dx * dx + dy * dy + dz * dz;
}

// One octant's line from the cell's stored list (cnt entries in ascending scene index; E has float members x, y, z and a fourth
// member w that holds the index bits).  ctr: the octant's centre; hb = h / 4: half its edge (the range test, against r, as the cell's
// own); hw: hb plus the slack of the cell's dominance box.  Keeps the entries within r of the octant box that none of the (up to)
// STOCS_OCTANT_K in-range entries nearest to the centre dominates over the widened box, writes the first STOCS_OCTANT_LINE of them to
// `line` in list order and, when there are 1..STOCS_OCTANT_LINE of them, pads the line with copies of the last.  Returns the number of
// survivors, counted up to STOCS_OCTANT_LINE + 1 (more than a line: the octant does not fit); 0 leaves the line untouched.
// Serial: one thread per (cell, octant) on the device -- the lists are a dozen entries long.
template <class E>
STOCS_OCT_HD uint32_t octant_line_build(const E* list, uint32_t cnt, const double ctr[3], double hb, double hw, double r, double margin, E* line) {
    const double r2 = r * r;
    // ---- the dominators: K rounds of "smallest (distance, position) key above the last one" over the in-range entries ----
    double dux[STOCS_OCTANT_K], duy[STOCS_OCTANT_K], duz[STOCS_OCTANT_K], dn2[STOCS_OCTANT_K];
    unsigned long long last = 0ull;
    int nd = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < STOCS_OCTANT_K; ++j) {
        dux[j] = 0.0; duy[j] = 0.0; duz[j] = 0.0; dn2[j] = 0.0;
        if (nd < j) continue;                                   // the in-range entries ran out in an earlier round
        unsigned long long best = ~0ull;
        double bx = 0.0, by = 0.0, bz = 0.0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const double px = (double)list[k].x, py = (double)list[k].y, pz = (double)list[k].z;
            if (!(octant_box_dist2(px, py, pz, ctr, hb) <= r2)) continue;
            const double ux = px - ctr[0], uy = py - ctr[1], uz = pz - ctr[2];
            const float d2 = (float)(ux * ux + uy * uy + uz * uz);   // (selection only: any entry is a valid dominator)
            uint32_t db;
            { union { float f; uint32_t u; } cv; cv.f = d2; db = cv.u; }
            const unsigned long long kk = ((unsigned long long)db << 32) | (unsigned long long)(k + 1u);
            if (kk > last && kk < best) { best = kk; bx = ux; by = uy; bz = uz; }
        }
        if (best == ~0ull) continue;
        last = best;
        dux[j] = bx; duy[j] = by; duz[j] = bz; dn2[j] = bx * bx + by * by + bz * bz;
        nd = j + 1;
    }
    // ---- every in-range entry against the dominators, survivors in list order ----
    uint32_t n = 0;
    for (uint32_t k = 0; k < cnt && n <= STOCS_OCTANT_LINE; ++k) {
        const E e = list[k];
        const double px = (double)e.x, py = (double)e.y, pz = (double)e.z;
        if (!(octant_box_dist2(px, py, pz, ctr, hb) <= r2)) continue;
        const double ux = px - ctr[0], uy = py - ctr[1], uz = pz - ctr[2];
        const double n2 = ux * ux + uy * uy + uz * uz;
        bool keep = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < STOCS_OCTANT_K; ++j)
            if (j < nd && dominated_over_box(n2, dn2[j], fabs(ux - dux[j]) + fabs(uy - duy[j]) + fabs(uz - duz[j]), hw, margin)) keep = false;   // (never by itself: 0 there)
        if (!keep) continue;
        if (n < STOCS_OCTANT_LINE) line[n] = e;
        n++;
    }
    if (n >= 1u && n <= STOCS_OCTANT_LINE)
        for (uint32_t k = n; k < STOCS_OCTANT_LINE; ++k) line[k] = line[n - 1u];
    return n;
}

}  // namespace stocs

#endif
