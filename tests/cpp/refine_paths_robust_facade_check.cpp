// The robust refinement behind the facade's batch and tracker (include/stocs.hpp): the run_trials and track_poses overloads that take
// keep_ratio and max_normal_deg, on a scene and a model given as flat clouds and a prior given as 12 floats (3x4 row-major).
//   refine_paths_robust_facade_check <scene.stcl> <model.stcl> <prior.txt>
// Checked here: with keep_ratio 1 and no gate either overload gives what the plain form gives, byte for byte, and with 0.7 / 30 degrees
// some refined pose differs from the plain one.  Printed for the caller to compare with the library's own results, floats as %.9g:
//   "batch <trial> <hypothesis> <base index> <refined lcp> <16 floats of the refined pose, column-major>"
//   "track <prior> <lcp> <refined lcp> <n_correspondences> <iterations> <16 floats of refined_pose16>"
// exit code 0 = all as expected
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <stocs.hpp>

#define CHECK(c) do { if (!(c)) { std::cerr << "failed: " #c << " (line " << __LINE__ << ") " << stocs_last_error() << std::endl; return 1; } } while (0)

static bool read_stcl(const std::string& path, std::vector<float>& pos, std::vector<float>& nrm, std::vector<float>* prob, std::vector<int32_t>* pixel) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[8];
    int32_t n = 0, flags = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && std::string(magic, 8) == "STOCSCL1" && fread(&n, 4, 1, f) == 1 && fread(&flags, 4, 1, f) == 1 && n >= 0;
    if (ok) {
        pos.resize((size_t)n * 3); nrm.resize((size_t)n * 3);
        ok = fread(pos.data(), 4, pos.size(), f) == pos.size() && fread(nrm.data(), 4, nrm.size(), f) == nrm.size();
        if (ok && (flags & 1)) { std::vector<float> p((size_t)n); ok = fread(p.data(), 4, (size_t)n, f) == (size_t)n; if (prob) *prob = p; }
        else if (prob) prob->assign((size_t)n, 1.0f);
        if (ok && (flags & 2)) { std::vector<int32_t> px((size_t)n * 2); ok = fread(px.data(), 4, px.size(), f) == px.size(); if (pixel) *pixel = px; }
    }
    fclose(f);
    return ok;
}

typedef std::vector<std::vector<PoseCandidate*> > Hyps;

// the refined hypotheses of a batch as bytes: lcp and transform of every one, trial by trial
static std::vector<float> flat(const Hyps& refined) {
    std::vector<float> v;
    for (size_t t = 0; t < refined.size(); ++t)
        for (size_t k = 0; k < refined[t].size(); ++k) {
            v.push_back(refined[t][k]->lcp);
            v.insert(v.end(), refined[t][k]->transform.data(), refined[t][k]->transform.data() + 16);
        }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::cerr << "usage: refine_paths_robust_facade_check <scene.stcl> <model.stcl> <prior.txt>" << std::endl; return 2; }
    stocs::SceneCloud scene;
    stocs::ModelCloud model;
    CHECK(read_stcl(argv[1], scene.pos, scene.nrm, &scene.class_probability, &scene.pixel));
    CHECK(read_stcl(argv[2], model.pos, model.nrm, NULL, NULL));
    MatrixType prior_m;   // identity; the bottom row stays 0 0 0 1
    {
        std::ifstream f(argv[3]);
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) { float v; CHECK(f >> v); prior_m(r, c) = v; }
    }
    stocs::stocs_estimator est(model, scene, std::string(), 640, 480, 0.005f, 5, 5, 0.0f, 0.10f);

    // ---- the batch: 4 trials from seed 5, the driver's clustering, 5 iterations at 3.5 cm ----
    stocs_trial_post post;
    post.acceptable_fraction = 0.8f; post.maximum_pose_count = 10; post.min_distance = 0.02f; post.min_angle = 15.0f;
    post.sym3[0] = post.sym3[1] = post.sym3[2] = 0.0f;
    post.refine_iterations = 5; post.max_correspondence_distance = 0.035f;
    std::vector<stocs::stocs_estimator::TrialResult> res;
    Hyps hyps, refined;
    const int best_plain = est.run_trials(4, 5, 100, 200, 0.9f, post, &res, &hyps, &refined);
    const std::vector<float> plain = flat(refined), plain_in = flat(hyps);
    CHECK(best_plain >= 0 && !plain.empty());
    CHECK(est.run_trials(4, 5, 100, 200, 0.9f, post, &res, &hyps, &refined, 1.0f, -1.0f) == best_plain);
    CHECK(flat(refined) == plain && flat(hyps) == plain_in);
    CHECK(est.run_trials(4, 5, 100, 200, 0.9f, post, &res, &hyps, &refined, 0.7f, 30.0f) == best_plain);
    const std::vector<float> robust = flat(refined);
    CHECK(flat(hyps) == plain_in && robust.size() == plain.size() && robust != plain);
    for (size_t t = 0; t < refined.size(); ++t)
        for (size_t k = 0; k < refined[t].size(); ++k) {
            printf("batch %d %d %d %.9g", (int)t, (int)k, (int)refined[t][k]->base_index, (double)refined[t][k]->lcp);
            for (int i = 0; i < 16; ++i) printf(" %.9g", (double)refined[t][k]->transform.data()[i]);
            printf("\n");
        }
    // an invalid setting is an error of the call: no pose, no hypotheses
    CHECK(est.run_trials(4, 5, 100, 200, 0.9f, post, &res, &hyps, &refined, 0.0f, 30.0f) == -1 && refined.empty());

    // ---- the tracker: the prior, two rounds of 64 samples, 5 iterations ----
    PoseCandidate prior(prior_m, 0.0f, -1.0f);
    std::vector<PoseCandidate*> priors(1, &prior);
    stocs_track_params prm = stocs::stocs_estimator::default_track_params();
    prm.rounds = 2; prm.samples = 64; prm.refine_iterations = 5;
    std::vector<stocs_track_result> a, b, c;
    CHECK(est.track_poses(priors, prm, &a).size() == 1 && a.size() == 1);
    CHECK(est.track_poses(priors, prm, 1.0f, -1.0f, &b).size() == 1 && b.size() == 1);
    CHECK(std::memcmp(&a[0], &b[0], sizeof(stocs_track_result)) == 0);
    CHECK(est.track_poses(priors, prm, 0.7f, 30.0f, &c).size() == 1 && c.size() == 1);
    CHECK(c[0].lcp == a[0].lcp && std::memcmp(c[0].pose16, a[0].pose16, 64) == 0);   // the rounds are the plain call's
    CHECK(std::memcmp(c[0].refined_pose16, a[0].refined_pose16, 64) != 0 && c[0].n_correspondences < a[0].n_correspondences);
    printf("track 0 %.9g %.9g %d %d", (double)c[0].lcp, (double)c[0].refined_lcp, (int)c[0].n_correspondences, (int)c[0].iterations);
    for (int i = 0; i < 16; ++i) printf(" %.9g", (double)c[0].refined_pose16[i]);
    printf("\n");
    CHECK(est.track_poses(priors, prm, 1.5f, 30.0f, &c).empty());
    return 0;
}
