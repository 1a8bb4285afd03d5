// octant_lists_check.cpp -- the octant lines of model_matching_amd/csrc/octant_lists.h on the host, against a brute-force scan.
// Compiled with g++ against the header alone (tests/test_octant_lists_cpu.py: plainly and under the address / undefined-behaviour
// sanitizers).  For a few hundred cells -- a randomly oriented surface patch sampled every 1.6-2 mm, or an exact lattice with
// duplicates (distances tie exactly) -- it restates what grid.hip builds: the points within r of the cell box, pruned by dominance over
// the widened cell box (the stored list, ascending index), then octant_line_build per octant.  10^4 positions per cell, a third of
// them with coordinates on the octant planes or one float next to them, are put in a cell and an octant by the kernel's own float
// floor; the nearest scene point under the product's rule (float distance x*x + (y*y + z*z) <= eps^2, ties to the larger index) over
// ALL points must be an entry of the position's octant line whenever that octant fits its line.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../model_matching_amd/csrc/octant_lists.h"

using namespace stocs;

struct Entry { float x, y, z, w; };   // as the device's float4: w holds the bits of the scene index

static float index_bits(int i) { float f; std::memcpy(&f, &i, 4); return f; }
static int bits_index(float f) { int i; std::memcpy(&i, &f, 4); return i; }

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } failures++; } } while (0)

int main() {
    // ---- the flag: pack / unpack round trip, octant of a quarter-cell coordinate ----
    {
        std::mt19937 rng(5);
        const uint32_t offs[] = {0u, 1u, 8u, 64u, 0x7FFFFFF8u, 0x7FFFFFFFu, 0x40000000u};
        for (uint32_t o : offs) {
            CHECK(!octant_word_flagged(o), "a plain offset %u reads as flagged", o);
            const uint32_t x = octant_word_pack(o);
            CHECK(octant_word_flagged(x) && octant_word_offset(x) == o, "pack / unpack of %u", o);
            for (uint32_t sc = 0; sc < 64; ++sc) CHECK(octant_line_offset(x, sc) == o + octant_line_start(sc), "line offset of %u, sub-cell %u", o, sc);
        }
        for (int k = 0; k < 100000; ++k) {
            const uint32_t o = rng() & 0x7FFFFFFFu;
            const uint32_t x = octant_word_pack(o);
            CHECK(octant_word_flagged(x) && octant_word_offset(x) == o && !octant_word_flagged(o), "pack / unpack of %u", o);
        }
        for (int s = 0; s < 64; ++s) {
            const int sx = s & 3, sy = (s >> 2) & 3, sz = s >> 4;
            const uint32_t want = (uint32_t)((sx >= 2) | ((sy >= 2) << 1) | ((sz >= 2) << 2));
            CHECK(octant_of_subcell((uint32_t)s) == want, "octant of sub-cell %d", s);
            // the line of a sub-cell is the line of its octant, a whole line inside the block, and no two octants share one
            const uint32_t ls = octant_line_start((uint32_t)s);
            CHECK(ls == octant_line_start_of_octant(want) && ls % 8u == 0u && ls < 64u, "line start %u of sub-cell %d", ls, s);
            for (uint32_t o2 = 0; o2 < 8; ++o2) CHECK((octant_line_start_of_octant(o2) == ls) == (o2 == want), "octants %u and %u share a line", o2, want);
            // whole cells added to the quarter-cell coordinates change nothing (also below the origin: arithmetic shifts)
            for (int c = -3; c <= 3; ++c) CHECK(octant_of_quarter(4 * c + sx, 4 * (c + 1) + sy, 4 * (c - 1) + sz) == want, "octant of quarter coordinates, sub-cell %d", s);
        }
    }

    // ---- the lines ----
    const double eps = 0.005, h = eps, r = 1.001 * eps;
    const float of[3] = {-0.0731f, -0.0402f, -0.0913f};            // the float origin the kernels subtract
    const float inv_h4 = (float)(1.0 / h) * 4.0f, sq_eps = (float)eps * (float)eps;
    const double ext = 0.4;                                        // extent of the grid the slack is sized for (grid.hip)
    const double hh = 0.5 * h + 2.0e-6 * (ext + 1.0) * 0.5 + 1.0e-7, reach = r + 2.0 * h, margin = 4.0e-6 * reach * reach;
    const double hw = 0.25 * h + (hh - 0.5 * h);
    std::mt19937_64 rng(2024);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const int n_cells = 300, n_pos = 10000;
    long octants = 0, fit = 0, long_cells = 0, checked = 0, on_plane = 0, no_neighbour = 0, line_entries = 0, stored_entries = 0;
    for (int cell = 0; cell < n_cells; ++cell) {
        const bool lattice = cell % 2 == 1;
        const int cc[3] = {(int)(rng() % 60) + 4, (int)(rng() % 60) + 4, (int)(rng() % 60) + 4};
        const double b0[3] = {of[0] + cc[0] * h, of[1] + cc[1] * h, of[2] + cc[2] * h};
        const double ctr[3] = {b0[0] + 0.5 * h, b0[1] + 0.5 * h, b0[2] + 0.5 * h};
        // ---- scene points around the cell, as floats ----
        std::vector<Entry> pts;
        if (lattice) {   // step 1.5625 mm on multiples of the step: exact in float, every midpoint ties; some exact duplicates behind
            const double a = 0.0015625;
            const int layers = 1 + (int)(rng() % 3);
            const long z0 = std::lround((ctr[2] + (U(rng) - 0.5) * 2.6 * h) / a);   // through the cell, or up to 0.8 h above / below it
            const int tilt = (int)(rng() % 3);      // 0: a flat sheet, 1 / 2: a staircase along x / y
            for (long ix = std::lround((ctr[0] - 1.7 * h) / a); ix * a <= ctr[0] + 1.7 * h; ++ix)
                for (long iy = std::lround((ctr[1] - 1.7 * h) / a); iy * a <= ctr[1] + 1.7 * h; ++iy)
                    for (int l = 0; l < layers; ++l) {
                        const long iz = z0 + l + (tilt == 1 ? ix / 2 : tilt == 2 ? iy / 3 : 0) - (tilt == 1 ? std::lround(ctr[0] / a) / 2 : tilt == 2 ? std::lround(ctr[1] / a) / 3 : 0);
                        pts.push_back({(float)(ix * a), (float)(iy * a), (float)(iz * a), 0.f});
                    }
            const size_t n0 = pts.size();
            for (int k = 0; k < 12; ++k) pts.push_back(pts[rng() % n0]);
        } else {         // a plane through the cell, jittered samples every 1.6-2 mm, a little noise off the plane
            double nrm[3] = {N(rng), N(rng), N(rng)};
            const double nl = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
            for (double& v : nrm) v /= nl;
            double t1[3] = {nrm[1], -nrm[0], 0.0};
            if (std::fabs(nrm[2]) > 0.9) { t1[0] = 0.0; t1[1] = nrm[2]; t1[2] = -nrm[1]; }
            const double tl = std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
            for (double& v : t1) v /= tl;
            const double t2[3] = {nrm[1] * t1[2] - nrm[2] * t1[1], nrm[2] * t1[0] - nrm[0] * t1[2], nrm[0] * t1[1] - nrm[1] * t1[0]};
            const double lift = (U(rng) - 0.5) * 2.6 * h;   // through the cell, or beside it within epsilon of it
            const double p0[3] = {ctr[0] + (U(rng) - 0.5) * h + lift * nrm[0], ctr[1] + (U(rng) - 0.5) * h + lift * nrm[1], ctr[2] + (U(rng) - 0.5) * h + lift * nrm[2]};
            const double step = 0.0016 + 0.0004 * U(rng);
            for (int i = -6; i <= 6; ++i)
                for (int j = -6; j <= 6; ++j) {
                    const double u = (i + 0.6 * (U(rng) - 0.5)) * step, v = (j + 0.6 * (U(rng) - 0.5)) * step, wn = 0.0002 * N(rng);
                    pts.push_back({(float)(p0[0] + u * t1[0] + v * t2[0] + wn * nrm[0]), (float)(p0[1] + u * t1[1] + v * t2[1] + wn * nrm[1]),
                                   (float)(p0[2] + u * t1[2] + v * t2[2] + wn * nrm[2]), 0.f});
                }
            std::shuffle(pts.begin(), pts.end(), rng);   // scene order is not spatial order
        }
        for (size_t i = 0; i < pts.size(); ++i) pts[i].w = index_bits((int)i);
        // ---- the cell's stored list: within r of the cell box, pruned over the widened cell box by the 8 entries nearest to the centre ----
        std::vector<Entry> inc;
        for (const Entry& e : pts)
            if (octant_box_dist2(e.x, e.y, e.z, ctr, 0.5 * h) <= r * r) inc.push_back(e);
        std::vector<std::pair<double, size_t>> byd;
        for (size_t k = 0; k < inc.size(); ++k) {
            const double ux = inc[k].x - ctr[0], uy = inc[k].y - ctr[1], uz = inc[k].z - ctr[2];
            byd.push_back({ux * ux + uy * uy + uz * uz, k});
        }
        std::sort(byd.begin(), byd.end());
        std::vector<Entry> stored;
        for (size_t k = 0; k < inc.size(); ++k) {
            const double ux = inc[k].x - ctr[0], uy = inc[k].y - ctr[1], uz = inc[k].z - ctr[2], n2 = ux * ux + uy * uy + uz * uz;
            bool keep = true;
            for (size_t j = 0; j < std::min<size_t>(8, byd.size()); ++j) {
                const Entry& d = inc[byd[j].second];
                const double vx = d.x - ctr[0], vy = d.y - ctr[1], vz = d.z - ctr[2];
                if (dominated_over_box(n2, vx * vx + vy * vy + vz * vz, std::fabs(ux - vx) + std::fabs(uy - vy) + std::fabs(uz - vz), hh, margin)) keep = false;
            }
            if (keep) stored.push_back(inc[k]);
        }
        stored_entries += (long)stored.size();
        if (stored.size() > 8) long_cells++;
        // ---- the eight lines (built for every cell here, whatever the length of its list: the claim does not depend on it) ----
        Entry lines[8][8];
        uint32_t nl[8];
        for (uint32_t o = 0; o < 8; ++o) {
            for (Entry& e : lines[o]) e = {1.0e30f, 1.0e30f, 1.0e30f, index_bits(-1)};   // the sentinel fill
            const double octr[3] = {b0[0] + (0.25 + 0.5 * (o & 1u)) * h, b0[1] + (0.25 + 0.5 * ((o >> 1) & 1u)) * h, b0[2] + (0.25 + 0.5 * (o >> 2)) * h};
            nl[o] = octant_line_build(stored.data(), (uint32_t)stored.size(), octr, 0.25 * h, hw, r, margin, lines[o]);
            octants++;
            if (nl[o] <= 8u) {
                fit++; line_entries += nl[o];
                for (uint32_t k = 1; k < 8 && nl[o]; ++k) {
                    const int i0 = bits_index(lines[o][k - 1].w), i1 = bits_index(lines[o][k].w);
                    CHECK(k < nl[o] ? i0 < i1 : i0 == i1, "cell %d octant %u: entries %d, %d at %u of %u are not ascending then padded", cell, o, i0, i1, k, nl[o]);
                }
            }
        }
        // ---- positions ----
        for (int t = 0; t < n_pos; ++t) {
            float q[3];
            bool plane = false;
            for (int a = 0; a < 3; ++a) {
                q[a] = (float)(b0[a] + U(rng) * h);
                if (t % 3 == 0 && rng() % 2) {   // on the octant plane of this axis, or one float below / above it
                    const float mid = (float)(b0[a] + 0.5 * h);
                    const int wch = (int)(rng() % 3);
                    q[a] = wch == 0 ? mid : (wch == 1 ? std::nextafterf(mid, -1.0e30f) : std::nextafterf(mid, 1.0e30f));
                    plane = true;
                }
            }
            // the kernel's cell and octant
            const int c4x = (int)std::floor((q[0] - of[0]) * inv_h4), c4y = (int)std::floor((q[1] - of[1]) * inv_h4), c4z = (int)std::floor((q[2] - of[2]) * inv_h4);
            if ((c4x >> 2) != cc[0] || (c4y >> 2) != cc[1] || (c4z >> 2) != cc[2]) continue;   // rounded into a neighbour cell: its lists answer
            const uint32_t o = octant_of_quarter(c4x, c4y, c4z);
            // brute force over every scene point, the product's tie rule
            float best = sq_eps; int bi = -1;
            for (const Entry& e : pts) {
                const float dx = q[0] - e.x, dy = q[1] - e.y, dz = q[2] - e.z;
                const float d = dx * dx + (dy * dy + dz * dz);
                if (d <= best) { best = d; bi = bits_index(e.w); }
            }
            if (bi < 0) { no_neighbour++; continue; }
            bool in_stored = false;
            for (const Entry& e : stored) in_stored |= bits_index(e.w) == bi;
            CHECK(in_stored, "cell %d: the nearest point %d of a position is not in the stored list", cell, bi);
            if (nl[o] > 8u) continue;          // this octant does not fit a line: its cell stays plain
            // what the kernel does with the line: 8 entries in order under `<=`
            float lb = sq_eps; int li = -1;
            for (const Entry& e : lines[o]) {
                const float dx = q[0] - e.x, dy = q[1] - e.y, dz = q[2] - e.z;
                const float d = dx * dx + (dy * dy + dz * dz);
                if (d <= lb) { lb = d; li = bits_index(e.w); }
            }
            CHECK(li == bi, "cell %d (%s) octant %u: the line answers %d, the scan over all points %d (position %.9g %.9g %.9g)", cell,
                  lattice ? "lattice" : "random", o, li, bi, q[0], q[1], q[2]);
            checked++;
            if (plane) on_plane++;
        }
    }
    std::printf("cells %d (long %ld), stored entries per cell %.2f, octants %ld, fitting a line %ld, entries per fitting line %.2f\n", n_cells, long_cells,
                (double)stored_entries / n_cells, octants, fit, fit ? (double)line_entries / (double)fit : 0.0);
    std::printf("positions checked %ld (on or next to an octant plane %ld), without a neighbour %ld\n", checked, on_plane, no_neighbour);
    // floors on what the run covered (a run in which nothing was pruned, nothing fitted or nothing was asked must not pass)
    CHECK(long_cells >= 100, "too few long cells: %ld", long_cells);
    CHECK(fit >= 800 && line_entries < 8 * fit, "too few octants fit a line, or none was pruned below a full line: %ld of %ld, %ld entries", fit, octants, line_entries);
    CHECK(checked >= 1000000 && on_plane >= 200000, "too few positions checked: %ld, %ld on planes", checked, on_plane);
    if (failures) { std::printf("octant_lists_check: %ld FAILED\n", failures); return 1; }
    std::printf("octant_lists_check: ok\n");
    return 0;
}
