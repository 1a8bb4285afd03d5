// The symmetry layer of the facade (include/stocs.hpp): stocs_estimator::symmetry_errors and find_symmetries, stocs::symmetry_close and
// stocs::find_symmetries_of, on a model with an exact four-fold axis about z (a seeded blade and its three quarter turns, which permute and
// negate the coordinates).  Every result is compared with the C ABI called directly on a context of its own.
//   symmetry_facade_check        exit code 0 = all as expected; prints "axes=<n> order=<o> K=<K> sym3=a,b,c flags=<f>"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>

#include <stocs.hpp>

#define CHECK(c) do { if (!(c)) { std::cerr << "failed: " #c << " (line " << __LINE__ << ") " << stocs_last_error() << std::endl; return 1; } } while (0)

int main() {
    stocs::ModelCloud model;
    uint32_t s = 12345u;
    for (int i = 0; i < 45; ++i) {   // the blade along +x: radius 0.012 .. 0.08, a narrow azimuth, height 0.8 r
        s = s * 1664525u + 1013904223u; const float r = 0.012f + 0.068f * (float)(s >> 8) / 16777216.0f;
        s = s * 1664525u + 1013904223u; const float phi = 0.05f * ((float)(s >> 8) / 16777216.0f - 0.5f);
        float p[3] = {r * std::cos(phi), r * std::sin(phi), 0.8f * r}, n[3] = {-0.6f, 0.0f, 0.8f};
        for (int k = 0; k < 4; ++k) {   // (x, y, z) -> (-y, x, z)
            model.pos.insert(model.pos.end(), p, p + 3); model.nrm.insert(model.nrm.end(), n, n + 3);
            const float px = -p[1], nx = -n[1];
            p[1] = p[0]; p[0] = px; n[1] = n[0]; n[0] = nx;
        }
    }
    stocs::SceneCloud scene;
    for (int i = 0; i < 32; ++i) {
        const float a = 0.2f * (float)i;
        const float p[3] = {0.05f * std::cos(a), 0.05f * std::sin(a), 0.8f + 0.001f * (float)i}, n[3] = {0.0f, 0.0f, -1.0f};
        scene.pos.insert(scene.pos.end(), p, p + 3); scene.nrm.insert(scene.nrm.end(), n, n + 3); scene.class_probability.push_back(1.0f);
    }
    stocs::stocs_estimator est(model, scene, std::string(), 640, 480, 0.005f, 5, 5, 0.5f, 0.1f);
    const float tol = 0.004f, z[3] = {0.0f, 0.0f, 1.0f};

    // symmetry_errors: the identity, a quarter turn (a symmetry), a turn by 45 degrees (not one)
    std::vector<float> T(48);
    CHECK(stocs_symmetry_rotation(z, 0.0, NULL, &T[0]) == STOCS_OK && stocs_symmetry_rotation(z, 90.0, NULL, &T[16]) == STOCS_OK &&
          stocs_symmetry_rotation(z, 45.0, NULL, &T[32]) == STOCS_OK);
    const std::vector<stocs_symmetry_error> rec = est.symmetry_errors(T, tol);
    CHECK(rec.size() == 3);
    CHECK(rec[0].sum_fix == 0 && rec[0].max == 0.0f && rec[0].n_far == 0 && rec[0].valid == 1);
    CHECK(rec[1].n_far == 0 && rec[1].max == 0.0f);
    CHECK(rec[2].n_far > 0);
    CHECK(est.symmetry_errors(std::vector<float>(), tol).empty());

    // the same through the C ABI on a context of its own
    const float sp[3] = {0, 0, 1}, sn[3] = {0, 0, -1}, spr[1] = {1.0f};
    stocs_params prm;
    stocs_default_params(&prm);
    stocs_ctx* ctx = NULL;
    CHECK(stocs_ctx_create(&prm, sp, sn, spr, NULL, 1, model.pos.data(), model.nrm.data(), model.size(), 0, -1, &ctx) == STOCS_OK);
    stocs_symmetry_params sprm;
    sprm.reach = tol; sprm.cos_normal = 0.8660254037844387f; sprm.reserved[0] = sprm.reserved[1] = 0;
    stocs_symmetry_error want[3];
    CHECK(stocs_symmetry_errors(ctx, T.data(), 3, &sprm, want) == STOCS_OK);
    CHECK(std::memcmp(want, rec.data(), sizeof want) == 0);

    // find_symmetries: the four-fold axis about z, the four turns, the descriptor (0, 0, 90)
    stocs_symmetry_search search = stocs::default_symmetry_search();
    search.tol_max = tol;
    const stocs::SymmetryResult r = est.find_symmetries(search);
    CHECK(r.ok && r.axes.size() == 1 && r.axes[0].order == 4 && std::fabs(r.axes[0].axis[2]) > 0.9999f);
    CHECK(r.set16.size() == 64 && r.flags == 0 && r.sym3[0] == 0.0f && r.sym3[1] == 0.0f && r.sym3[2] == 90.0f);
    const stocs::SymmetryResult w = stocs::find_symmetries_of(ctx, search, NULL);
    CHECK(w.ok && w.axes.size() == r.axes.size() && std::memcmp(w.axes.data(), r.axes.data(), sizeof(stocs_symmetry_axis)) == 0);
    CHECK(w.set16 == r.set16 && w.flags == r.flags);
    stocs_ctx_destroy(ctx);

    // symmetry_close: the generator's closure is the found set's size; a cap below it truncates
    const std::vector<float> gen(T.begin() + 16, T.begin() + 32);
    bool truncated = true;
    const std::vector<float> closed = stocs::symmetry_close(gen, 1.0f, STOCS_POSE_SYM_MAX, &truncated);
    CHECK(closed.size() == 64 && !truncated && std::memcmp(closed.data(), T.data(), 64) == 0);
    CHECK(stocs::symmetry_close(gen, 1.0f, 3, &truncated).size() == 48 && truncated);
    CHECK(stocs::symmetry_close(gen, 1.0f, 0).empty());
    printf("axes=%zu order=%d K=%zu sym3=%g,%g,%g flags=%d\n", r.axes.size(), r.axes[0].order, r.set16.size() / 16, (double)r.sym3[0], (double)r.sym3[1],
           (double)r.sym3[2], r.flags);
    return 0;
}
