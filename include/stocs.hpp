// stocs.hpp -- drop-in C++ façade: the public surface of the reference's include/stocs.hpp (+ the types of
// include/point3d.hpp and the few rgbd:: helpers its driver uses), implemented on the C ABI of libstocs_hip.so
// (include/stocs_hip.h).  Header-only; needs no Eigen / PCL / OpenCV / Boost.
//
// A caller written against the reference -- src/stocs_match_one_object.cpp:51-215, src/model_preprocess.cpp:14-39 --
// compiles against this header unchanged: same class name, same constructor argument list (reference stocs.hpp:18-30),
// same method names, argument order and error behaviour (bool returns, NULL best pose, no exceptions from the hot
// path; only construction throws because a constructor cannot return a status), same global type names
// (Point3D, Quadrilateral, PoseCandidate, PPFMapType, MatrixType, VectorType, micro).  tests/cpp/reference_call_sequence.cpp
// is that call sequence, restated.
//
// What differs, and why (INTEGRATION.md has the table):
//   * Eigen::Matrix4f -> stocs::Mat4f (16 floats, column-major = Eigen::Matrix4f::data() layout, operator()(r, c));
//     Eigen::Vector3f -> stocs::Vec3f;
//   * PPFMapType is a handle to this repo's flat index file (written by stocs::pre_process_model), not a std::map: the
//     reference's 128-fold map does not fit memory beyond toy models (3.2e9 entries at |M| = 5000); rgbd::load_ppf_map
//     fills the handle, the estimator loads the index straight onto the GPU;
//   * files: PNG (8/16-bit, non-interlaced) and PLY (ascii / binary little endian) through the library's own readers;
//   * draws are seeded (set_seed) instead of clock-seeded (divergence Q6); PoseCandidate objects are owned by the
//     estimator and freed with it (the reference leaks them);
//   * batched methods (sample_bases / find_congruent_sets_all / make_transforms) exist next to the per-call ones: they
//     are what apps/stocs_single.cpp uses -- one GPU pass over all bases instead of one round trip per base.
#ifndef STOCS_FACADE_HPP
#define STOCS_FACADE_HPP

#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "stocs_hip.h"

namespace stocs {

struct Vec3f {   // stands in for Eigen::Matrix<float, 3, 1>
    float v[3];
    Vec3f() { v[0] = v[1] = v[2] = 0.0f; }
    Vec3f(float x, float y, float z) { v[0] = x; v[1] = y; v[2] = z; }
    float operator[](int i) const { return v[i]; }
    float& operator[](int i) { return v[i]; }
    float operator()(int i) const { return v[i]; }
    float& operator()(int i) { return v[i]; }
    float x() const { return v[0]; }
    float y() const { return v[1]; }
    float z() const { return v[2]; }
    float squaredNorm() const { return v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]); }
    float norm() const { return std::sqrt(squaredNorm()); }
    Vec3f normalized() const { const float z = squaredNorm(); if (z > 0.0f) { const float s = std::sqrt(z); return Vec3f(v[0] / s, v[1] / s, v[2] / s); } return *this; }
    Vec3f operator-(const Vec3f& o) const { return Vec3f(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
    Vec3f operator+(const Vec3f& o) const { return Vec3f(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
    const float* data() const { return v; }
    float* data() { return v; }
};

struct Mat4f {  // column-major, layout-compatible with Eigen::Matrix4f::data()
    float m[16];
    Mat4f() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = m[15] = 1.0f; }
    float operator()(int r, int c) const { return m[c * 4 + r]; }
    float& operator()(int r, int c) { return m[c * 4 + r]; }
    const float* data() const { return m; }
    float* data() { return m; }
};

}  // namespace stocs

// ---- global names of the reference's headers (point3d.hpp:11-156, stocs.hpp:8-12, rgbd.hpp:23-26) ----
using Scalar = float;
using VectorType = stocs::Vec3f;
using MatrixType = stocs::Mat4f;
static constexpr Scalar kLargeNumber = 1e9;
using micro = std::chrono::microseconds;

class Point3D {   // reference include/point3d.hpp:11-92
public:
    using Scalar = float;
    using VectorType = stocs::Vec3f;
    Point3D(Scalar x, Scalar y, Scalar z) : pos_(x, y, z), rgb_(-1.0f, -1.0f, -1.0f), pixel_(0, 0), class_probability_(0), edge_probability_(0), current_probability_(0) {}
    explicit Point3D(const VectorType& other) : Point3D(other[0], other[1], other[2]) {}
    Point3D() : Point3D(0.0f, 0.0f, 0.0f) {}
    VectorType& pos() { return pos_; }
    const VectorType& pos() const { return pos_; }
    const VectorType& rgb() const { return rgb_; }
    const float& probability() const { return current_probability_; }
    const float& class_probability() const { return class_probability_; }
    const std::pair<int, int>& pixel() const { return pixel_; }
    const VectorType& normal() const { return normal_; }
    void set_rgb(const VectorType& rgb) { rgb_ = rgb; }
    void set_normal(const VectorType& normal) { normal_ = normal.normalized(); }
    void set_pixel(const std::pair<int, int>& pixel) { pixel_ = pixel; }
    void set_probability(float class_probability, float edge_probability) {
        class_probability_ = class_probability; edge_probability_ = edge_probability; current_probability_ = class_probability;
    }
    void update_class_probability(float decay_fraction) { class_probability_ = decay_fraction * class_probability_; }
    void update_probability(float new_probability) { current_probability_ = new_probability; }
    void reset_probability() { current_probability_ = class_probability_; }
    bool hasColor() const { return rgb_.squaredNorm() > Scalar(0.001); }
    Scalar& x() { return pos_.v[0]; }
    Scalar& y() { return pos_.v[1]; }
    Scalar& z() { return pos_.v[2]; }
    Scalar x() const { return pos_.v[0]; }
    Scalar y() const { return pos_.v[1]; }
    Scalar z() const { return pos_.v[2]; }
private:
    VectorType pos_, normal_, rgb_;
    std::pair<int, int> pixel_;
    float class_probability_, edge_probability_, current_probability_;
};

struct Quadrilateral {   // reference include/point3d.hpp:116-139
    std::array<int, 4> vertices;
    Quadrilateral(int v0, int v1, int v2, int v3) { vertices = {{v0, v1, v2, v3}}; }
    bool operator<(const Quadrilateral& rhs) const { return vertices < rhs.vertices; }
    bool operator==(const Quadrilateral& rhs) const { return vertices == rhs.vertices; }
    int operator[](int idx) const { return vertices[idx]; }
    int& operator[](int idx) { return vertices[idx]; }
};

class PoseCandidate {   // reference include/point3d.hpp:141-156
public:
    MatrixType transform;  // camera frame
    float lcp;
    int base_index;
    PoseCandidate(MatrixType transform, float lcp, float base_index) {
        this->transform = transform; this->lcp = lcp; this->base_index = (int)base_index;
    }
    ~PoseCandidate() {}
};

// The model's PPF index as callers hold it between rgbd::load_ppf_map and the estimator (reference rgbd.hpp:23:
// std::map<std::vector<int>, std::vector<std::pair<int,int>>>).  Here: where the flat index file lives.
struct PPFMapType {
    std::string location;   // empty: no file, the estimator builds the index on the GPU at construction
    int64_t n_pairs = 0;
    size_t size() const { return (size_t)n_pairs; }
    bool empty() const { return location.empty(); }
};

namespace stocs {
using ::Quadrilateral;
using ::PoseCandidate;
using ::Point3D;
using ::PPFMapType;

inline bool file_exists(const std::string& p) { struct stat b; return stat(p.c_str(), &b) == 0; }

struct ModelCloud {
    std::vector<float> pos;  // 3 floats per point (model_search.ply of the reference)
    std::vector<float> nrm;
    int size() const { return (int)(pos.size() / 3); }
};

struct SceneCloud {  // what rgbd::load_rgbd_data_sampled produces (reference src/rgbd.cpp:179-281)
    std::vector<float> pos, nrm, class_probability;
    std::vector<int32_t> pixel;       // row, col per point (may be empty)
    std::vector<uint8_t> edge_map;    // image_height*image_width png values, empty when no edge.png
    int size() const { return (int)(pos.size() / 3); }
};

// one image file -> samples (throws on failure)
template <class T>
inline void read_image(const std::string& path, int want_channels, int want_bits, int width, int height, std::vector<T>* out) {
    int w = 0, h = 0, c = 0, b = 0;
    if (stocs_png_read(path.c_str(), &w, &h, &c, &b, NULL, 0) != STOCS_OK) throw std::runtime_error(std::string("stocs_png_read: ") + stocs_last_error());
    if (c != want_channels || b != want_bits || (width > 0 && (w != width || h != height)))
        throw std::runtime_error(path + ": expected a " + std::to_string(width) + "x" + std::to_string(height) + " " + std::to_string(want_bits) + "-bit image with " +
                                 std::to_string(want_channels) + " channel(s)");
    out->resize((size_t)w * h * c);
    if (stocs_png_read(path.c_str(), &w, &h, &c, &b, out->data(), (int64_t)(out->size() * sizeof(T))) != STOCS_OK)
        throw std::runtime_error(std::string("stocs_png_read: ") + stocs_last_error());
}

inline void read_ply(const std::string& path, ModelCloud* m, bool need_normals) {
    int n = 0, hn = 0;
    if (stocs_ply_read(path.c_str(), NULL, NULL, 0, &n, &hn) != STOCS_OK) throw std::runtime_error(std::string("stocs_ply_read: ") + stocs_last_error());
    if (need_normals && !hn) throw std::runtime_error(path + ": no normals (run pre_process_model first)");
    m->pos.resize((size_t)n * 3); m->nrm.resize((size_t)n * 3);
    if (stocs_ply_read(path.c_str(), m->pos.data(), m->nrm.data(), n, &n, &hn) != STOCS_OK) throw std::runtime_error(std::string("stocs_ply_read: ") + stocs_last_error());
    if (need_normals) {   // rgbd::load_ply_model (rgbd.cpp:12-33): points without a finite normal are dropped
        size_t w = 0;
        for (int i = 0; i < n; ++i) {
            const float* q = &m->nrm[(size_t)i * 3];
            if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]))) continue;
            for (int k = 0; k < 3; ++k) { m->pos[w * 3 + k] = m->pos[(size_t)i * 3 + k]; m->nrm[w * 3 + k] = q[k]; }
            ++w;
        }
        m->pos.resize(w * 3); m->nrm.resize(w * 3);
    }
}

}  // namespace stocs

namespace rgbd {   // the helpers of reference include/rgbd.hpp a caller of the estimator touches

// rgbd.cpp:166-177: the reference deserialises a Boost archive into a std::map; here the handle records where the flat
// index file is (the estimator loads it onto the GPU) and how many pairs it holds
inline void load_ppf_map(std::string ppf_map_location, PPFMapType& ppf_map) {
    ppf_map.location.clear(); ppf_map.n_pairs = 0;
    FILE* f = fopen(ppf_map_location.c_str(), "rb");
    if (!f) return;
    char magic[8];
    int32_t hdr[6];
    int64_t counts[2];
    if (fread(magic, 1, 8, f) == 8 && !memcmp(magic, "STOCSIX1", 8) && fread(hdr, 4, 6, f) == 6 && fread(counts, 8, 2, f) == 2) {
        ppf_map.location = ppf_map_location;
        ppf_map.n_pairs = counts[1];
    }
    fclose(f);
}

// rgbd.cpp:35-56
inline void save_as_ply(std::string location, std::vector<Point3D>& point3d, float scale) {
    std::vector<float> p(point3d.size() * 3), n(point3d.size() * 3);
    for (size_t i = 0; i < point3d.size(); ++i)
        for (int k = 0; k < 3; ++k) { p[3 * i + k] = point3d[i].pos()[k]; n[3 * i + k] = point3d[i].normal()[k]; }
    (void)stocs_ply_write(location.c_str(), p.data(), n.data(), (int)point3d.size(), scale);
}

// rgbd.cpp:58-70
inline void transform_pointset(std::vector<Point3D>& input, std::vector<Point3D>& output, MatrixType& transform) {
    for (size_t i = 0; i < input.size(); ++i) {
        const VectorType& p = input[i].pos();
        const MatrixType& t = transform;
        output.push_back(Point3D(((t(0, 0) * p[0] + t(0, 1) * p[1]) + t(0, 2) * p[2]) + t(0, 3), ((t(1, 0) * p[0] + t(1, 1) * p[1]) + t(1, 2) * p[2]) + t(1, 3),
                                 ((t(2, 0) * p[0] + t(2, 1) * p[1]) + t(2, 2) * p[2]) + t(2, 3)));
    }
}

}  // namespace rgbd

namespace stocs {

// Not in the reference: what stocs_find_symmetries reports.  axes best first (order 0: continuous); set16 the K x 16 floats of the closed
// set for pose_errors_sym (entry 0 the identity); sym3 the clustering descriptor, zeros when flags carries
// STOCS_SYMMETRY_DESCRIPTOR_INEXACT; STOCS_SYMMETRY_SET_TRUNCATED / STOCS_SYMMETRY_NOTHING_FOUND as the header says.
struct SymmetryResult {
    bool ok;
    std::vector<stocs_symmetry_axis> axes;
    std::vector<float> set16;
    float sym3[3];
    int flags;
};
inline stocs_symmetry_search default_symmetry_search() {
    stocs_symmetry_search s;
    stocs_default_symmetry_search(&s);
    return s;
}
inline SymmetryResult find_symmetries_of(stocs_ctx* ctx, const stocs_symmetry_search& search, const float* center3) {
    SymmetryResult r;
    r.ok = false; r.flags = 0; r.sym3[0] = r.sym3[1] = r.sym3[2] = 0.0f;
    const int cap_axes = search.n_refine > 0 ? search.n_refine : 1;
    r.axes.resize((size_t)cap_axes);
    r.set16.resize((size_t)STOCS_POSE_SYM_MAX * 16);
    int n = 0, K = 0;
    if (stocs_find_symmetries(ctx, &search, center3, r.axes.data(), cap_axes, &n, r.set16.data(), STOCS_POSE_SYM_MAX, &K, r.sym3, &r.flags) != STOCS_OK) {
        r.axes.clear(); r.set16.clear();
        return r;
    }
    r.axes.resize((size_t)(n < cap_axes ? n : cap_axes));
    r.set16.resize((size_t)K * 16);
    r.ok = true;
    return r;
}

class stocs_estimator {
public:
    // reference stocs.hpp:18-61, argument for argument
    stocs_estimator(std::string model_location, PPFMapType& ppf_map_preloaded, std::string rgb_location, std::string depth_location,
                    std::string class_probability_map_location, std::string edge_probability_map_location, std::string debug_location,
                    std::vector<float> camera_intrinsics, int image_width, int image_height, float read_depth_scale, float write_depth_scale,
                    float voxel_size, float distance_threshold, int ppf_tr_discretization, int ppf_rot_discretization, float edge_threshold,
                    float class_threshold) {
        reset_members(debug_location, image_width, image_height, distance_threshold, ppf_tr_discretization, ppf_rot_discretization, edge_threshold, class_threshold);
        load_object_info(model_location, ppf_map_preloaded);
        load_scene_info(rgb_location, depth_location, class_probability_map_location, edge_probability_map_location, camera_intrinsics, read_depth_scale,
                        write_depth_scale, voxel_size, debug_location + "/sampled_scene.ply");
        create_context(-1);
        centroid_shift();       // both happen inside stocs_ctx_create; kept for callers that spell them out
        kdtree_initialize();
    }
    // the same with the images already in memory (row-major, image_height x image_width; edge may be NULL)
    stocs_estimator(const ModelCloud& model, PPFMapType& ppf_map_preloaded, const uint16_t* depth, const uint16_t* class_probability_map,
                    const uint8_t* edge_probability_map, std::string debug_location, std::vector<float> camera_intrinsics, int image_width,
                    int image_height, float read_depth_scale, float write_depth_scale, float voxel_size, float distance_threshold,
                    int ppf_tr_discretization, int ppf_rot_discretization, float edge_threshold, float class_threshold, int device = -1) {
        reset_members(debug_location, image_width, image_height, distance_threshold, ppf_tr_discretization, ppf_rot_discretization, edge_threshold, class_threshold);
        model_ = model;
        ppf_location_ = ppf_map_preloaded.location;
        ingest(depth, class_probability_map, edge_probability_map, camera_intrinsics, read_depth_scale, write_depth_scale, voxel_size, std::string());
        create_context(device);
    }
    // clouds already sampled (tests, callers with their own ingest); the index is built on the GPU
    stocs_estimator(const ModelCloud& model, const SceneCloud& scene, std::string debug_location, int image_width, int image_height,
                    float distance_threshold, int ppf_tr_discretization, int ppf_rot_discretization, float edge_threshold, float class_threshold,
                    int device = -1) {
        reset_members(debug_location, image_width, image_height, distance_threshold, ppf_tr_discretization, ppf_rot_discretization, edge_threshold, class_threshold);
        model_ = model;
        scene_ = scene;
        create_context(device);
    }
    // not in the reference: one object of a frame ingested for several (load_frame_scenes), with the object's preloaded PPF index.
    // log: where the estimator's own lines go (std::cout when NULL) -- several estimators on host threads each keep theirs apart.
    stocs_estimator(const ModelCloud& model, PPFMapType& ppf_map_preloaded, const SceneCloud& scene, std::string debug_location, int image_width,
                    int image_height, float distance_threshold, int ppf_tr_discretization, int ppf_rot_discretization, float edge_threshold,
                    float class_threshold, int device = -1, std::ostream* log = NULL) {
        reset_members(debug_location, image_width, image_height, distance_threshold, ppf_tr_discretization, ppf_rot_discretization, edge_threshold, class_threshold);
        if (log) log_ = log;
        model_ = model;
        ppf_location_ = ppf_map_preloaded.location;
        scene_ = scene;
        create_context(device);
    }
    ~stocs_estimator() { stocs_ctx_destroy(ctx_); }
    stocs_estimator(const stocs_estimator&) = delete;
    stocs_estimator& operator=(const stocs_estimator&) = delete;

    // reference stocs.hpp:65-67 / stocs.cpp:86-97: model_search.ply + the preloaded index handle
    void load_object_info(std::string model_location, PPFMapType& ppf_map_preloaded) {
        read_ply(model_location, &model_, true);
        ppf_location_ = ppf_map_preloaded.location;
        *log_ << "|M| = " << model_.size() << ",  |map(M)| = " << ppf_map_preloaded.size() << std::endl;
    }
    // reference stocs.hpp:69-78 / stocs.cpp:99-131 -> rgbd::load_rgbd_data_sampled (rgbd.cpp:179-281), on the GPU.  The
    // rgb image only colours the reference's debug clouds and is not read.
    void load_scene_info(std::string rgb_location, std::string depth_location, std::string class_probability_map_location,
                         std::string edge_probability_map_location, std::vector<float> camera_intrinsics, float read_depth_scale, float write_depth_scale,
                         float voxel_size, std::string dst_scene_location) {
        (void)rgb_location;
        std::vector<uint16_t> depth, prob;
        std::vector<uint8_t> edge;
        read_image(depth_location, 1, 16, image_width, image_height, &depth);
        read_image(class_probability_map_location, 1, 16, image_width, image_height, &prob);
        const bool has_edge = file_exists(edge_probability_map_location);   // stat(), stocs.cpp:115
        if (has_edge) read_image(edge_probability_map_location, 1, 8, image_width, image_height, &edge);
        ingest(depth.data(), prob.data(), has_edge ? edge.data() : NULL, camera_intrinsics, read_depth_scale, write_depth_scale, voxel_size, dst_scene_location);
    }

    void set_seed(uint64_t seed) { seed_ = seed; attempt_ = 0; la_n_ = 0; la_in_ctx_ = false; }
    // Extension, no reference counterpart: with `on`, a nearest-neighbour query whose closest scene points lie at exactly the same
    // float32 distance takes the point the reference's kd-tree returns instead of the one with the largest index (stocs_set_option
    // "exact_ties", include/stocs_hip.h; divergence Q11).  Every score and pose then follows the reference's integer answers exactly;
    // it costs a kd-tree build per scene and a slower scoring kernel.  Off by default.
    void set_exact_ties(bool on) {
        const int rc = stocs_set_option(ctx_, "exact_ties", on ? 1 : 0);
        if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_set_option(exact_ties): ") + stocs_last_error());
    }
    // not in the reference (one estimator per scene there): the next frame against the same model; the model
    // clouds and the PPF index are kept, everything derived from the old scene is dropped
    void set_scene(const SceneCloud& scene) {
        scene_ = scene;
        const int rc = stocs_ctx_set_scene(ctx_, scene_.pos.data(), scene_.nrm.data(), scene_.class_probability.data(),
                                           scene_.pixel.empty() ? NULL : scene_.pixel.data(), scene_.size());
        if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_ctx_set_scene: ") + stocs_last_error());
        if (!scene_.edge_map.empty()) stocs_set_edge_map(ctx_, scene_.edge_map.data());
        attempt_ = 0; best_lcp = 0; best_index = -1; la_n_ = 0; la_in_ctx_ = false;
        all_transforms.clear(); all_pose.clear(); all_pose_store_.clear(); batched_ = false;
    }
    bool has_edge_map() const { return !scene_.edge_map.empty(); }
    stocs_ctx* context() { return ctx_; }
    int scene_size() const { return scene_.size(); }
    int model_size() const { return model_.size(); }

    // reference stocs.hpp:80-83 / stocs.cpp:363-519
    bool sample_class_base(std::vector<int>& base_indices, float& invariant1, float& invariant2) {
        return sample_one(0, 0.0f, base_indices, invariant1, invariant2);
    }
    // reference stocs.hpp:85-91 / stocs.cpp:559-751; `segment` receives the survivors of pass 1 inside the mask (:628-638)
    bool sample_instance_base(std::vector<int>& base_indices, float& invariant1, float& invariant2, std::vector<Point3D>& segment, float dispersion,
                              int base_num) {
        attempt_ = base_num - 1;
        const bool ok = sample_one(1, dispersion, base_indices, invariant1, invariant2);
        int n = 0;
        if (stocs_get_segment(ctx_, NULL, 0, &n) == STOCS_OK && n > 0) {
            std::vector<int32_t> idx((size_t)n);
            stocs_get_segment(ctx_, idx.data(), n, &n);
            const std::vector<Point3D>& sc = scene_points();
            for (int i = 0; i < n; ++i) segment.push_back(sc[(size_t)idx[i]]);
        }
        return ok;
    }

    // reference stocs.hpp:93-96 / stocs.cpp:753-869
    bool find_congruent_sets_on_model(std::vector<int>& base_indices, float invariant1, float invariant2, std::vector<Quadrilateral>* quadrilaterals) {
        quadrilaterals->clear();
        const int32_t ids[4] = {base_indices[0], base_indices[1], base_indices[2], base_indices[3]};
        const float inv[2] = {invariant1, invariant2};
        int64_t total = 0, n = 0;
        int slot = lookahead_slot(ids, inv);
        if (slot >= 0) {                // one of the bases the facade sampled ahead: one search for all of them, then only read-backs
            if (!la_congruent_done_) {
                if (stocs_find_congruent_all(ctx_, &total) != STOCS_OK) return false;
                la_congruent_done_ = true;
            }
            if (stocs_get_quads(ctx_, slot, NULL, 0, &total) != STOCS_OK) return false;
        } else {
            la_in_ctx_ = false;
            slot = 0;
            if (stocs_set_bases(ctx_, 1, ids, inv) != STOCS_OK || stocs_find_congruent_all(ctx_, &total) != STOCS_OK) return false;
        }
        std::vector<int32_t> q((size_t)total * 4 + 4);
        if (stocs_get_quads(ctx_, slot, q.data(), total, &n) != STOCS_OK) return false;
        for (int64_t i = 0; i < n; ++i) quadrilaterals->emplace_back(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
        return quadrilaterals->size() != 0;
    }

    // reference stocs.hpp:98-101 / stocs.cpp:871-941: appends (centred transform, camera-frame pose)
    bool get_rigid_transform_from_congruent_pair(std::vector<int>& base_indices, Quadrilateral& congruent_quad, int base_index) {
        const int32_t ids[4] = {base_indices[0], base_indices[1], base_indices[2], base_indices[3]};
        const int32_t q[4] = {congruent_quad[0], congruent_quad[1], congruent_quad[2], congruent_quad[3]};
        Mat4f T, P;
        int ok = 0;
        if (stocs_rigid_transform(ctx_, ids, q, T.data(), P.data(), &ok) == STOCS_OK && ok) {
            if (batched_) { all_transforms.clear(); all_pose.clear(); all_pose_store_.clear(); batched_ = false; }
            all_transforms.push_back(T);
            all_pose_store_.emplace_back(new PoseCandidate(P, 0, (float)base_index));
            all_pose.push_back(all_pose_store_.back().get());
        }
        return true;  // the reference always returns true (stocs.cpp:940)
    }

    // reference stocs.hpp:103-104 / stocs.cpp:1006-1041
    Scalar compute_alignment_score_for_rigid_transform(const MatrixType& mat) {
        float s = 0;
        stocs_score_transforms(ctx_, mat.data(), 1, &s);
        return s;
    }

    // reference stocs.hpp:106-107 / stocs.cpp:982-1004 (batched on the GPU; first maximum wins)
    void compute_best_transform() {
        if (batched_) {   // candidates live on the device (make_transforms): score + arg-max there, one round trip
            float pose[16];
            *log_ << "Transforms to verify: " << n_batched_ << std::endl;   // stocs.cpp:985
            if (stocs_verify_all(ctx_, &best_lcp, &best_index, pose) != STOCS_OK) {
                // the reference's error convention: text on stdout, "no pose" state, no exception from the hot path
                *log_ << "compute_best_transform failed: " << stocs_last_error() << std::endl;
                best_lcp = 0;
                best_index = -1;
            }
            *log_ << "best index: " << best_index << ", maximum score: " << best_lcp << std::endl;   // :1003
            fetched_ = false;
            return;
        }
        const int n = (int)all_transforms.size();
        *log_ << "Transforms to verify: " << n << std::endl;
        std::vector<float> T((size_t)n * 16), l((size_t)n);
        for (int i = 0; i < n; ++i) std::memcpy(&T[(size_t)i * 16], all_transforms[(size_t)i].data(), 64);
        Scalar max_score = 0;
        int index = -1;
        if (n > 0 && stocs_score_transforms(ctx_, T.data(), n, l.data()) == STOCS_OK) {
            for (int i = 0; i < n; ++i) {
                all_pose[(size_t)i]->lcp = l[(size_t)i];
                if (l[(size_t)i] > max_score) { max_score = l[(size_t)i]; index = i; }
            }
        }
        best_lcp = max_score;
        best_index = index;
        *log_ << "best index: " << best_index << ", maximum score: " << best_lcp << std::endl;
    }

    // reference stocs.hpp:109-113: run by the constructor there; here both are part of stocs_ctx_create (sequential f32
    // centroid sums, scene grid on the GPU), so these are idempotent no-ops kept for callers that name them
    void kdtree_initialize() {}
    void centroid_shift() {}

    VectorType get_scene_centroid() { Vec3f c; stocs_get_centroids(ctx_, c.v, NULL); return c; }
    std::vector<PoseCandidate*> get_pose_candidates() { fetch_batched(); return all_pose; }
    Scalar get_best_score() { return best_lcp; }
    int get_best_index() const { return best_index; }   // not in the reference: index of get_best_pose() in get_pose_candidates(), -1 if none
    PoseCandidate* get_best_pose() {
        if (best_index == -1) return NULL;
        fetch_batched();
        return all_pose[(size_t)best_index];
    }
    const std::vector<MatrixType>& get_all_transforms() { fetch_batched(); return all_transforms; }

    // reference stocs.hpp:136-149: the model under the best (centred-frame) transform and the scene, as PLY files
    void visualize_best_pose() {
        if (best_index == -1) return;
        fetch_batched();
        std::vector<Point3D> point3d_model_pose, model_pts = model_points_centred();
        rgbd::transform_pointset(model_pts, point3d_model_pose, all_transforms[(size_t)best_index]);
        rgbd::save_as_ply(debug_location + "/best_pose.ply", point3d_model_pose, 1);
        std::vector<Point3D> sc = scene_points();
        rgbd::save_as_ply(debug_location + "/scene.ply", sc, 1);
    }

    // ---- batched forms of the caller's loops (stocs_match_one_object.cpp:81-147), one GPU pass each ----
    // n attempts of sample_class_base / sample_instance_base (by the presence of the edge map, :90); valid bases are kept
    int sample_bases(int n_attempts, float dispersion) {
        base_ids_.assign((size_t)n_attempts * 4, -1); base_inv_.assign((size_t)n_attempts * 2, 0.0f); base_valid_.assign((size_t)n_attempts, 0);
        la_n_ = 0; la_in_ctx_ = false;
        if (stocs_clear_bases(ctx_) != STOCS_OK) return 0;
        if (stocs_sample_bases(ctx_, has_edge_map() ? 1 : 0, seed_, 0, n_attempts, dispersion, base_ids_.data(), base_inv_.data(), base_valid_.data()) != STOCS_OK) return 0;
        return stocs_num_bases(ctx_);
    }
    // find_congruent_sets_on_model for every sampled base; returns the total number of congruent sets
    long long find_congruent_sets_all() {
        int64_t total = 0;
        return stocs_find_congruent_all(ctx_, &total) == STOCS_OK ? (long long)total : -1;
    }
    // the <= maximum_congruent_sets loop (:120-147) with the library's seeded subset rule; returns the candidate count
    int make_transforms(int maximum_congruent_sets) {
        int n = 0;
        if (stocs_make_transforms(ctx_, maximum_congruent_sets, seed_, &n) != STOCS_OK) return -1;
        batched_ = true; fetched_ = false; n_batched_ = n;
        return n;
    }

    // N independent runs of that whole loop (base attempts -> congruent sets -> <= maximum_congruent_sets transforms per base ->
    // compute_best_transform) with seeds first_seed, first_seed + 1, ... in ONE set of GPU launches (stocs_run_trials): what
    // BASELINE config 4 ("64 parallel StoCS trials") runs.  Trial t equals, bit for bit, the run a fresh estimator with
    // set_seed(first_seed + t) gives through the three calls above + compute_best_transform.  The best trial's pose becomes the
    // estimator's best pose (get_best_score / get_best_pose); returns the index of that trial, -1 when no trial found a pose.
    struct TrialResult { int n_bases, n_candidates; long long n_congruent_sets; float best_lcp; int best_index; MatrixType best_pose; };
    int run_trials(int n_trials, uint64_t first_seed, int number_of_bases, int maximum_congruent_sets, float dispersion, std::vector<TrialResult>* results = NULL) {
        return run_trials_impl(n_trials, first_seed, number_of_bases, maximum_congruent_sets, dispersion, NULL, results);
    }
    // the same batch with post-processing inside it (stocs_run_trials_post): every trial's candidates clustered on the device
    // (clustering::greedy_clustering with post's fraction, count, distance, angle and sym_info, best_score = the trial's best lcp) and,
    // with post.refine_iterations > 0, the kept hypotheses refined (clustering::point_to_plane_icp on the whole scene) and rescored.
    // hypotheses[t]: trial t's kept candidates (camera-frame transform, lcp, base index) in cluster order; refined[t]: the same
    // hypotheses refined (refined transform, rescored lcp) -- the candidates themselves without refinement.  Owned by the estimator
    // until the next run_trials.
    int run_trials(int n_trials, uint64_t first_seed, int number_of_bases, int maximum_congruent_sets, float dispersion, const stocs_trial_post& post,
                   std::vector<TrialResult>* results, std::vector<std::vector<PoseCandidate*> >* hypotheses,
                   std::vector<std::vector<PoseCandidate*> >* refined = NULL) {
        return run_trials_post_impl(n_trials, first_seed, number_of_bases, maximum_congruent_sets, dispersion, post, NULL, results, hypotheses, refined);
    }
    // ... with the kept hypotheses refined by the robust form inside the batch (stocs_run_trials_post_robust): keep_ratio and
    // max_normal_deg as refine_pose_candidates_robust takes them (< 0: no gate; the angle becomes a cosine once:
    // (float)cos((double)deg * pi / 180)).  keep_ratio = 1 and no gate: bitwise the form above.
    int run_trials(int n_trials, uint64_t first_seed, int number_of_bases, int maximum_congruent_sets, float dispersion, const stocs_trial_post& post,
                   std::vector<TrialResult>* results, std::vector<std::vector<PoseCandidate*> >* hypotheses,
                   std::vector<std::vector<PoseCandidate*> >* refined, float keep_ratio, float max_normal_deg) {
        const float robust[2] = {keep_ratio, robust_min_cos(max_normal_deg)};
        return run_trials_post_impl(n_trials, first_seed, number_of_bases, maximum_congruent_sets, dispersion, post, robust, results, hypotheses, refined);
    }
    // degrees -> the min_normal_cos of the robust entry points: one conversion, the cosine in double (< 0: gate off)
    static float robust_min_cos(float max_normal_deg) {
        return max_normal_deg >= 0.0f ? (float)std::cos((double)max_normal_deg * 3.141592653589793 / 180.0) : -2.0f;
    }

private:
    // robust: NULL, or (keep_ratio, min_normal_cos)
    int run_trials_post_impl(int n_trials, uint64_t first_seed, int number_of_bases, int maximum_congruent_sets, float dispersion, const stocs_trial_post& post,
                             const float* robust, std::vector<TrialResult>* results, std::vector<std::vector<PoseCandidate*> >* hypotheses,
                             std::vector<std::vector<PoseCandidate*> >* refined) {
        hyp_store_.clear();
        if (hypotheses) hypotheses->clear();
        if (refined) refined->clear();
        const int best = run_trials_impl(n_trials, first_seed, number_of_bases, maximum_congruent_sets, dispersion, &post, results, robust);
        if (best == -2) return -1;
        std::vector<stocs_trial_hypothesis> h;
        for (int t = 0; t < n_trials; ++t) {
            int n = 0;
            if (stocs_trials_get_hypotheses(ctx_, t, NULL, 0, &n) != STOCS_OK) return -1;
            h.resize((size_t)std::max(n, 1));
            if (n > 0 && stocs_trials_get_hypotheses(ctx_, t, h.data(), n, &n) != STOCS_OK) return -1;
            std::vector<PoseCandidate*> a, b;
            for (int i = 0; i < n; ++i) {
                MatrixType m, r;
                memcpy(m.data(), h[(size_t)i].pose16, 64);
                memcpy(r.data(), h[(size_t)i].refined_pose16, 64);
                hyp_store_.emplace_back(new PoseCandidate(m, h[(size_t)i].lcp, (float)h[(size_t)i].base_index));
                a.push_back(hyp_store_.back().get());
                hyp_store_.emplace_back(new PoseCandidate(r, h[(size_t)i].refined_lcp, (float)h[(size_t)i].base_index));
                b.push_back(hyp_store_.back().get());
            }
            if (hypotheses) hypotheses->push_back(a);
            if (refined) refined->push_back(b);
        }
        return best;
    }

    // -2: the library call failed (the public forms return -1 then, as for "no pose")
    int run_trials_impl(int n_trials, uint64_t first_seed, int number_of_bases, int maximum_congruent_sets, float dispersion, const stocs_trial_post* post,
                        std::vector<TrialResult>* results, const float* robust = NULL) {
        std::vector<uint64_t> seeds((size_t)std::max(n_trials, 0));
        for (int t = 0; t < n_trials; ++t) seeds[(size_t)t] = first_seed + (uint64_t)t;
        std::vector<stocs_trial_result> r((size_t)std::max(n_trials, 1));
        la_n_ = 0; la_in_ctx_ = false; batched_ = false; fetched_ = false; n_batched_ = 0;
        const int rc = post && robust ? stocs_run_trials_post_robust(ctx_, has_edge_map() ? 1 : 0, n_trials, seeds.data(), number_of_bases, dispersion,
                                                                     maximum_congruent_sets, 0, post, robust[0], robust[1], r.data())
                       : post ? stocs_run_trials_post(ctx_, has_edge_map() ? 1 : 0, n_trials, seeds.data(), number_of_bases, dispersion, maximum_congruent_sets, 0,
                                                    post, r.data())
                            : stocs_run_trials(ctx_, has_edge_map() ? 1 : 0, n_trials, seeds.data(), number_of_bases, dispersion, maximum_congruent_sets, 0, r.data());
        if (rc != STOCS_OK) return post ? -2 : -1;
        int best = -1;
        if (results) results->clear();
        for (int t = 0; t < n_trials; ++t) {
            if (r[(size_t)t].best_index >= 0 && (best < 0 || r[(size_t)t].best_lcp > r[(size_t)best].best_lcp)) best = t;   // strict >: the first best trial wins
            if (results) {
                TrialResult x;
                x.n_bases = r[(size_t)t].n_bases; x.n_candidates = r[(size_t)t].n_candidates; x.n_congruent_sets = (long long)r[(size_t)t].n_quads;
                x.best_lcp = r[(size_t)t].best_lcp; x.best_index = r[(size_t)t].best_index;
                memcpy(x.best_pose.data(), r[(size_t)t].best_pose16, 64);
                results->push_back(x);
            }
        }
        trial_best_.reset();
        best_lcp = 0; best_index = -1;
        if (best >= 0) {
            MatrixType m;
            memcpy(m.data(), r[(size_t)best].best_pose16, 64);
            trial_best_.reset(new PoseCandidate(m, r[(size_t)best].best_lcp, -1.0f));
            best_lcp = r[(size_t)best].best_lcp;
        }
        return best;
    }

public:
    // the winner of the last run_trials (camera frame), NULL when no trial found a pose; owned by the estimator
    PoseCandidate* get_best_trial_pose() const { return trial_best_.get(); }

    // clustering::point_to_plane_icp (reference pose_clustering.cpp:123-140) for every hypothesis at once, on the estimator's own scene
    // and model (stocs_refine_poses): the camera-frame hypotheses go to the centred frame, are refined against every scene point and
    // rescored.  Returns new candidates (camera-frame refined transform, rescored lcp, the input's base_index) in input order, owned by
    // the estimator until the next call; empty on error (the text is on stdout, as compute_best_transform reports errors).
    std::vector<PoseCandidate*> refine_pose_candidates(const std::vector<PoseCandidate*>& hypotheses, int max_iterations = 5,
                                                       float max_correspondence_distance = 0.035f) {
        refined_store_.clear();
        std::vector<PoseCandidate*> out;
        const int n = (int)hypotheses.size();
        float cs[3], cm[3];
        stocs_get_centroids(ctx_, cs, cm);
        std::vector<float> T((size_t)n * 16), P((size_t)n * 16), l((size_t)n);
        for (int i = 0; i < n; ++i) {
            // camera -> centred: same linear part, t = (t_camera - c_scene) + R c_model (in double, rounded once)
            const float* src = hypotheses[(size_t)i]->transform.data();
            float* dst = &T[(size_t)i * 16];
            std::memcpy(dst, src, 64);
            for (int r = 0; r < 3; ++r)
                dst[12 + r] = (float)(((double)src[12 + r] - (double)cs[r]) +
                                      (((double)src[r] * (double)cm[0] + (double)src[4 + r] * (double)cm[1]) + (double)src[8 + r] * (double)cm[2]));
        }
        if (n > 0 && stocs_refine_poses(ctx_, T.data(), n, NULL, 0, max_iterations, max_correspondence_distance, NULL, P.data(), l.data(), NULL, NULL) != STOCS_OK) {
            *log_ << "refine_pose_candidates failed: " << stocs_last_error() << std::endl;
            return out;
        }
        for (int i = 0; i < n; ++i) {
            MatrixType m;
            std::memcpy(m.data(), &P[(size_t)i * 16], 64);
            refined_store_.emplace_back(new PoseCandidate(m, l[(size_t)i], (float)hypotheses[(size_t)i]->base_index));
            out.push_back(refined_store_.back().get());
        }
        return out;
    }

    // The robust form of refine_pose_candidates (stocs_refine_poses_robust; the reference declares clustering::trimmed_icp and never
    // defines it): per iteration only the nearest keep_ratio of the candidate pairs enter the system, and with max_normal_deg >= 0 a
    // pair whose normals differ by more than that angle is no candidate (< 0: no gate; the angle becomes a cosine once:
    // (float)cos((double)deg * pi / 180)).  keep_ratio = 1 and no gate: bitwise refine_pose_candidates.  Same frame conversion, ownership
    // and error reporting as refine_pose_candidates; the two calls share one result store.
    std::vector<PoseCandidate*> refine_pose_candidates_robust(const std::vector<PoseCandidate*>& hypotheses, int max_iterations = 5,
                                                              float max_correspondence_distance = 0.035f, float keep_ratio = 0.7f,
                                                              float max_normal_deg = 30.0f) {
        refined_store_.clear();
        std::vector<PoseCandidate*> out;
        const int n = (int)hypotheses.size();
        float cs[3], cm[3];
        stocs_get_centroids(ctx_, cs, cm);
        std::vector<float> T((size_t)n * 16), P((size_t)n * 16), l((size_t)n);
        for (int i = 0; i < n; ++i) {
            const float* src = hypotheses[(size_t)i]->transform.data();
            float* dst = &T[(size_t)i * 16];
            std::memcpy(dst, src, 64);
            for (int r = 0; r < 3; ++r)
                dst[12 + r] = (float)(((double)src[12 + r] - (double)cs[r]) +
                                      (((double)src[r] * (double)cm[0] + (double)src[4 + r] * (double)cm[1]) + (double)src[8 + r] * (double)cm[2]));
        }
        stocs_refine_robust_params prm;
        prm.max_iterations = max_iterations; prm.max_correspondence_distance = max_correspondence_distance; prm.keep_ratio = keep_ratio;
        prm.min_normal_cos = robust_min_cos(max_normal_deg);
        if (n > 0 && stocs_refine_poses_robust(ctx_, T.data(), n, NULL, 0, &prm, NULL, P.data(), l.data(), NULL, NULL, NULL) != STOCS_OK) {
            *log_ << "refine_pose_candidates_robust failed: " << stocs_last_error() << std::endl;
            return out;
        }
        for (int i = 0; i < n; ++i) {
            MatrixType m;
            std::memcpy(m.data(), &P[(size_t)i * 16], 64);
            refined_store_.emplace_back(new PoseCandidate(m, l[(size_t)i], (float)hypotheses[(size_t)i]->base_index));
            out.push_back(refined_store_.back().get());
        }
        return out;
    }

    // Tracking across frames (stocs_track_poses; no reference counterpart): the defaults of a local search around a prior pose
    // (model_matching_amd/estimator.py TRACK_DEFAULTS, chosen by tools/track_time.py's sweep)
    static stocs_track_params default_track_params() {
        stocs_track_params p;
        p.rounds = 6; p.samples = 2048; p.max_translation = 0.02f; p.max_rotation_deg = 10.0f; p.shrink = 0.7f; p.seed = 0;
        p.refine_iterations = 0; p.max_correspondence_distance = 0.035f; p.keep_details = 0;
        return p;
    }
    // The camera-frame priors (e.g. the previous frame's poses) searched around on this estimator's current scene.  Returns one new
    // candidate per prior, owned by the estimator until the next call: the better of the search's pose and the refined pose (the search
    // pose on a tie), with its lcp and the prior's base_index; results (may be NULL) receives the raw records.  Empty on error (the
    // text goes to the log, as compute_best_transform reports errors).
    std::vector<PoseCandidate*> track_poses(const std::vector<PoseCandidate*>& priors, const stocs_track_params& prm = default_track_params(),
                                            std::vector<stocs_track_result>* results = NULL) {
        return track_poses_impl(priors, prm, NULL, results);
    }
    // ... with the final incumbents refined by the robust form (stocs_track_poses_robust): keep_ratio and max_normal_deg as
    // refine_pose_candidates_robust takes them (< 0: no gate).  keep_ratio = 1 and no gate: bitwise the form above.
    std::vector<PoseCandidate*> track_poses(const std::vector<PoseCandidate*>& priors, const stocs_track_params& prm, float keep_ratio, float max_normal_deg,
                                            std::vector<stocs_track_result>* results = NULL) {
        const float robust[2] = {keep_ratio, robust_min_cos(max_normal_deg)};
        return track_poses_impl(priors, prm, robust, results);
    }

private:
    std::vector<PoseCandidate*> track_poses_impl(const std::vector<PoseCandidate*>& priors, const stocs_track_params& prm, const float* robust,
                                                 std::vector<stocs_track_result>* results) {
        tracked_store_.clear();
        std::vector<PoseCandidate*> out;
        const int n = (int)priors.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], priors[(size_t)i]->transform.data(), 64);
        std::vector<stocs_track_result> r((size_t)std::max(n, 1));
        if (n > 0 && (robust ? stocs_track_poses_robust(ctx_, P.data(), n, &prm, robust[0], robust[1], r.data()) : stocs_track_poses(ctx_, P.data(), n, &prm, r.data())) != STOCS_OK) {
            *log_ << "track_poses failed: " << stocs_last_error() << std::endl;
            return out;
        }
        r.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            const stocs_track_result& t = r[(size_t)i];
            const bool ref = t.refined_lcp > t.lcp;
            MatrixType m;
            std::memcpy(m.data(), ref ? t.refined_pose16 : t.pose16, 64);
            tracked_store_.emplace_back(new PoseCandidate(m, ref ? t.refined_lcp : t.lcp, (float)priors[(size_t)i]->base_index));
            out.push_back(tracked_store_.back().get());
        }
        if (results) *results = r;
        return out;
    }

public:
    // Depth-image verification (stocs_ctx_set_frame / stocs_depth_check_poses; no reference counterpart): the camera frame this
    // estimator's scene came from -- depth and, optionally, the object's class-probability image (may be NULL), image_height x
    // image_width, row-major -- handed to the context once; then any number of camera-frame hypotheses (get_pose_candidates, the
    // hypotheses of run_trials, track_poses' results) are scored against it in one GPU pass: one record per hypothesis, in input
    // order.  Empty on error (the text goes to the log).
    static stocs_depth_params default_depth_params() {
        stocs_depth_params p;
        stocs_default_depth_params(&p);
        return p;
    }
    void set_frame(const uint16_t* depth, const uint16_t* class_probability_map, const std::vector<float>& camera_intrinsics, float read_depth_scale) {
        if (camera_intrinsics.size() < 4) throw std::runtime_error("camera_intrinsics must hold {fx, cx, fy, cy}");
        stocs_camera cam;
        cam.fx = camera_intrinsics[0]; cam.cx = camera_intrinsics[1]; cam.fy = camera_intrinsics[2]; cam.cy = camera_intrinsics[3];
        cam.depth_scale = read_depth_scale; cam.width = image_width; cam.height = image_height; cam.normal_method = STOCS_NORMALS_DEPTH_GRADIENT;
        if (stocs_ctx_set_frame(ctx_, &cam, depth, class_probability_map) != STOCS_OK) throw std::runtime_error(std::string("stocs_ctx_set_frame: ") + stocs_last_error());
    }
    std::vector<stocs_depth_result> depth_check_poses(const std::vector<PoseCandidate*>& poses, const stocs_depth_params& prm = default_depth_params()) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<stocs_depth_result> r((size_t)n);
        if (n > 0 && stocs_depth_check_poses(ctx_, P.data(), n, &prm, r.data()) != STOCS_OK) {
            *log_ << "depth_check_poses failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }

    // Pose errors against ground truth (stocs_pose_errors / stocs_model_diameter; no reference counterpart): the camera-frame estimates
    // against one ground-truth pose (gt.size() == 1) or one each (gt.size() == est.size()), in one GPU pass: ADD, ADD-S and their maxima
    // in metres, one record per estimate in input order.  Empty on error (the text goes to the log).  model_diameter: the largest
    // distance between two model points, computed on the device once; negative on error.
    std::vector<stocs_pose_error> pose_errors(const std::vector<PoseCandidate*>& est, const std::vector<PoseCandidate*>& gt) {
        const int n = (int)est.size(), n_gt = (int)gt.size();
        std::vector<float> P((size_t)n * 16), G((size_t)n_gt * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], est[(size_t)i]->transform.data(), 64);
        for (int i = 0; i < n_gt; ++i) std::memcpy(&G[(size_t)i * 16], gt[(size_t)i]->transform.data(), 64);
        std::vector<stocs_pose_error> r((size_t)n);
        if (n > 0 && stocs_pose_errors(ctx_, P.data(), n, G.data(), n_gt, r.data()) != STOCS_OK) {
            *log_ << "pose_errors failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    // Pose errors under model symmetries (stocs_pose_errors_sym; no reference counterpart): as pose_errors, under the K symmetry transforms
    // of the model frame in sym16 (K x 16 floats, column-major; symmetry_set below builds them from a clustering descriptor): MSSD and
    // symmetric ADD in metres and, with a camera (only fx, cx, fy, cy are read), MSPD in pixels, with the symmetry that attains each.  Empty
    // on error (the text goes to the log).
    std::vector<stocs_pose_error_sym> pose_errors_sym(const std::vector<PoseCandidate*>& est, const std::vector<PoseCandidate*>& gt, const std::vector<float>& sym16,
                                                      const stocs_camera* cam = NULL) {
        const int n = (int)est.size(), n_gt = (int)gt.size();
        std::vector<float> P((size_t)n * 16), G((size_t)n_gt * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], est[(size_t)i]->transform.data(), 64);
        for (int i = 0; i < n_gt; ++i) std::memcpy(&G[(size_t)i * 16], gt[(size_t)i]->transform.data(), 64);
        std::vector<stocs_pose_error_sym> r((size_t)n);
        if (n > 0 && stocs_pose_errors_sym(ctx_, P.data(), n, G.data(), n_gt, sym16.data(), (int)(sym16.size() / 16), cam, r.data()) != STOCS_OK) {
            *log_ << "pose_errors_sym failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    // The model under K transforms of its own frame against itself (stocs_symmetry_errors; no reference counterpart): sym16 holds K x 16
    // floats, column-major; reach is the largest distance at which a transformed point still has a neighbour.  One record per transform.
    // Empty on error (the text goes to the log).
    std::vector<stocs_symmetry_error> symmetry_errors(const std::vector<float>& sym16, float reach, float cos_normal = 0.8660254037844387f) {
        const int K = (int)(sym16.size() / 16);
        stocs_symmetry_params p;
        p.reach = reach; p.cos_normal = cos_normal; p.reserved[0] = p.reserved[1] = 0;
        std::vector<stocs_symmetry_error> r((size_t)K);
        if (K > 0 && stocs_symmetry_errors(ctx_, sym16.data(), K, &p, r.data()) != STOCS_OK) {
            *log_ << "symmetry_errors failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    // The model's symmetry axes and the set they generate (stocs_find_symmetries): see SymmetryResult above the class.  ok == false on error (the
    // text goes to the log).  center3 NULL: the model's centroid.
    SymmetryResult find_symmetries(const stocs_symmetry_search& search = default_symmetry_search(), const float* center3 = NULL) {
        SymmetryResult r = find_symmetries_of(ctx_, search, center3);
        if (!r.ok) *log_ << "find_symmetries failed: " << stocs_last_error() << std::endl;
        return r;
    }
    float model_diameter() {
        float d = -1.0f;
        if (stocs_model_diameter(ctx_, &d) != STOCS_OK) {
            *log_ << "model_diameter failed: " << stocs_last_error() << std::endl;
            return -1.0f;
        }
        return d;
    }

    // Visible-surface discrepancy (stocs_pose_errors_vsd / stocs_render_depth; no reference counterpart): the camera-frame estimates
    // against ground truth (one pose or one each, as pose_errors) on the frame of set_frame, each rendered as surfels and compared only
    // where it is visible in the depth image: BOP's third measure, which needs no symmetry set.  default_vsd_params fills BOP's ten taus,
    // 0.05, 0.10 .. 0.50 model diameters (n_tau stays 0 when the diameter fails).  render_depth: the z image of every pose, image_height x
    // image_width floats each, 0 where empty.  Empty on error (the text goes to the log).
    stocs_vsd_params default_vsd_params() {
        stocs_vsd_params p;
        stocs_default_vsd_params(&p);
        const float d = model_diameter();
        if (d > 0.0f) {
            p.n_tau = 10;
            for (int i = 0; i < 10; ++i) p.tau[i] = (float)(0.05 * (i + 1)) * d;
        }
        return p;
    }
    std::vector<stocs_vsd_record> pose_errors_vsd(const std::vector<PoseCandidate*>& est, const std::vector<PoseCandidate*>& gt, const stocs_vsd_params& prm) {
        const int n = (int)est.size(), n_gt = (int)gt.size();
        std::vector<float> P((size_t)n * 16), G((size_t)n_gt * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], est[(size_t)i]->transform.data(), 64);
        for (int i = 0; i < n_gt; ++i) std::memcpy(&G[(size_t)i * 16], gt[(size_t)i]->transform.data(), 64);
        std::vector<stocs_vsd_record> r((size_t)n);
        if (n > 0 && stocs_pose_errors_vsd(ctx_, P.data(), n, G.data(), n_gt, &prm, r.data()) != STOCS_OK) {
            *log_ << "pose_errors_vsd failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    std::vector<float> render_depth(const std::vector<PoseCandidate*>& poses, const stocs_vsd_params& prm) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<float> z((size_t)n * (size_t)image_width * (size_t)image_height);
        if (n > 0 && stocs_render_depth(ctx_, P.data(), n, &prm, z.data()) != STOCS_OK) {
            *log_ << "render_depth failed: " << stocs_last_error() << std::endl;
            z.clear();
        }
        return z;
    }
    // The model as a triangle mesh (stocs_ctx_set_mesh; no reference counterpart): vertices (3 floats each) and triangles (3 indices
    // each) in the frame of the model cloud; kept on the device until the next call, no triangles drops it.  render_depth_mesh and
    // pose_errors_vsd_mesh are render_depth and pose_errors_vsd with the mesh rasterised exactly in place of the surfels (the two
    // surfel fields of the parameters are not read).  false / empty on error (the text goes to the log).
    bool set_mesh(const std::vector<float>& vertices3, const std::vector<int32_t>& triangles3) {
        if (stocs_ctx_set_mesh(ctx_, vertices3.data(), (int)(vertices3.size() / 3), triangles3.data(), (int)(triangles3.size() / 3)) != STOCS_OK) {
            *log_ << "set_mesh failed: " << stocs_last_error() << std::endl;
            return false;
        }
        return true;
    }
    std::vector<stocs_vsd_record> pose_errors_vsd_mesh(const std::vector<PoseCandidate*>& est, const std::vector<PoseCandidate*>& gt, const stocs_vsd_params& prm) {
        const int n = (int)est.size(), n_gt = (int)gt.size();
        std::vector<float> P((size_t)n * 16), G((size_t)n_gt * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], est[(size_t)i]->transform.data(), 64);
        for (int i = 0; i < n_gt; ++i) std::memcpy(&G[(size_t)i * 16], gt[(size_t)i]->transform.data(), 64);
        std::vector<stocs_vsd_record> r((size_t)n);
        if (n > 0 && stocs_pose_errors_vsd_mesh(ctx_, P.data(), n, G.data(), n_gt, &prm, r.data()) != STOCS_OK) {
            *log_ << "pose_errors_vsd_mesh failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    std::vector<float> render_depth_mesh(const std::vector<PoseCandidate*>& poses) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<float> z((size_t)n * (size_t)image_width * (size_t)image_height);
        if (n > 0 && stocs_render_depth_mesh(ctx_, P.data(), n, z.data()) != STOCS_OK) {
            *log_ << "render_depth_mesh failed: " << stocs_last_error() << std::endl;
            z.clear();
        }
        return z;
    }

    // Joint rendering (stocs_explain_poses; no reference counterpart): the camera-frame poses -- the instances select_instances kept, say
    // -- rendered TOGETHER against the frame of set_frame, nearest surface first: one record per pose in input order (footprint,
    // visible / hidden behind the others, and the visible pixels' agreement with the depth image), and, when `labels` is given, the
    // image_height x image_width label image (-1: nobody, else the pose's index) with its per-pixel state when `state` is given too.
    // Empty on error (the text goes to the log).
    static stocs_render_params default_render_params() {
        stocs_render_params p;
        stocs_default_render_params(&p);
        return p;
    }
    std::vector<stocs_render_result> explain_poses(const std::vector<PoseCandidate*>& poses, std::vector<int32_t>* labels = NULL,
                                                   std::vector<uint8_t>* state = NULL, const stocs_render_params& prm = default_render_params()) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<stocs_render_result> r((size_t)n);
        const size_t npix = (size_t)image_width * (size_t)image_height;
        if (labels) labels->assign(npix, -1);
        if (labels && state) state->assign(npix, 0);
        if (stocs_explain_poses(ctx_, P.data(), n, &prm, r.data(), labels ? labels->data() : NULL, labels && state ? state->data() : NULL) != STOCS_OK) {
            *log_ << "explain_poses failed: " << stocs_last_error() << std::endl;
            r.clear();
            if (labels) labels->clear();
            if (state) state->clear();
        }
        return r;
    }

    // explain_poses on the mesh of set_mesh (stocs_explain_poses_mesh): the same records, labels and state from the exact surface; of prm
    // only tolerance and class_threshold are read.  Empty on error (the text goes to the log).
    std::vector<stocs_render_result> explain_poses_mesh(const std::vector<PoseCandidate*>& poses, std::vector<int32_t>* labels = NULL,
                                                        std::vector<uint8_t>* state = NULL, const stocs_render_params& prm = default_render_params()) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<stocs_render_result> r((size_t)n);
        const size_t npix = (size_t)image_width * (size_t)image_height;
        if (labels) labels->assign(npix, -1);
        if (labels && state) state->assign(npix, 0);
        if (stocs_explain_poses_mesh(ctx_, P.data(), n, &prm, r.data(), labels ? labels->data() : NULL, labels && state ? state->data() : NULL) != STOCS_OK) {
            *log_ << "explain_poses_mesh failed: " << stocs_last_error() << std::endl;
            r.clear();
            if (labels) labels->clear();
            if (state) state->clear();
        }
        return r;
    }

private:
    // What the three refine_poses_visible* methods share: the poses marshalled to 16 floats each, call(P, n, Q, records, trace rows or
    // NULL), on failure the log line and everything empty, else the `refined` copy.  K: max_iterations, for the trace's K + 1 rows a pose.
    template <class Record, class Call>
    std::vector<Record> refine_visible_with(const char* name, const std::vector<PoseCandidate*>& poses, std::vector<MatrixType>* refined,
                                            std::vector<stocs_refine_visible_trace>* trace, int K, Call call) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16), Q((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<Record> r((size_t)n);
        if (refined) refined->assign((size_t)n, MatrixType());
        if (trace) trace->assign((size_t)n * (size_t)(K > 0 ? K + 1 : 1), stocs_refine_visible_trace());
        if (n > 0 && call(P.data(), n, Q.data(), r.data(), trace ? trace->data() : NULL) != STOCS_OK) {
            *log_ << name << " failed: " << stocs_last_error() << std::endl;
            r.clear();
            if (refined) refined->clear();
            if (trace) trace->clear();
            return r;
        }
        for (int i = 0; refined && i < n; ++i) std::memcpy((*refined)[(size_t)i].data(), &Q[(size_t)i * 16], 64);
        return r;
    }

public:
    // Refinement on the visible surface (stocs_refine_poses_visible; no reference counterpart): the camera-frame poses refined against the
    // frame of set_frame on the surface of the mesh of set_mesh that each pose shows, projective point-to-plane on every depth pixel under
    // the rendered silhouette.  One record per pose in input order, describing the last evaluation; `refined` (when given) receives the
    // poses, a pose that could not be refined as it came.  max_iterations 0 scores the poses and changes nothing.  Empty on error (the
    // text goes to the log).
    static stocs_refine_visible_params default_refine_visible_params() {
        stocs_refine_visible_params p;
        stocs_default_refine_visible_params(&p);
        return p;
    }
    std::vector<stocs_refine_visible_result> refine_poses_visible(const std::vector<PoseCandidate*>& poses, std::vector<MatrixType>* refined = NULL,
                                                                  const stocs_refine_visible_params& prm = default_refine_visible_params()) {
        return refine_visible_with<stocs_refine_visible_result>("refine_poses_visible", poses, refined, NULL, 0,
            [&](const float* P, int n, float* Q, stocs_refine_visible_result* r, stocs_refine_visible_trace*) { return stocs_refine_poses_visible(ctx_, P, n, &prm, Q, r); });
    }

    // Damped refinement on the visible surface (stocs_refine_poses_visible_damped; no reference counterpart): refine_poses_visible with
    // Levenberg-Marquardt steps that are bounded, turn about a point of the object (prm.pivot_model, in the model frame) and are taken only
    // when they lower the cost, so a pose never comes back with a higher cost than it came with.  One record per pose in input order,
    // describing the RETURNED pose; `refined` (when given) receives the poses.  Empty on error (the text goes to the log).
    static stocs_refine_visible_damped_params default_refine_visible_damped_params() {
        stocs_refine_visible_damped_params p;
        stocs_default_refine_visible_damped_params(&p);
        return p;
    }
    std::vector<stocs_refine_visible_damped_result> refine_poses_visible_damped(const std::vector<PoseCandidate*>& poses, std::vector<MatrixType>* refined = NULL,
                                                                                const stocs_refine_visible_damped_params& prm = default_refine_visible_damped_params(),
                                                                                std::vector<stocs_refine_visible_trace>* trace = NULL) {
        return refine_visible_with<stocs_refine_visible_damped_result>("refine_poses_visible_damped", poses, refined, trace, prm.base.max_iterations,
            [&](const float* P, int n, float* Q, stocs_refine_visible_damped_result* r, stocs_refine_visible_trace* t) { return stocs_refine_poses_visible_damped(ctx_, P, n, &prm, Q, r, t); });
    }

    // Damped refinement with the contour term (stocs_refine_poses_visible_contour; no reference counterpart): refine_poses_visible_damped
    // in which the frame's object pixels (the class image of set_frame) that a pose's render leaves uncovered pull the pose towards them,
    // each paired with the nearest silhouette pixel within prm.pull_radius_px, and a pose that sheds object pixels pays for each.  One
    // record per pose in input order, describing the RETURNED pose; `refined` (when given) receives the poses.  Empty on error (the text
    // goes to the log); a frame without a class image is an error.
    static stocs_refine_visible_contour_params default_refine_visible_contour_params() {
        stocs_refine_visible_contour_params p;
        stocs_default_refine_visible_contour_params(&p);
        return p;
    }
    std::vector<stocs_refine_visible_contour_result> refine_poses_visible_contour(const std::vector<PoseCandidate*>& poses, std::vector<MatrixType>* refined = NULL,
                                                                                  const stocs_refine_visible_contour_params& prm = default_refine_visible_contour_params(),
                                                                                  std::vector<stocs_refine_visible_trace>* trace = NULL) {
        return refine_visible_with<stocs_refine_visible_contour_result>("refine_poses_visible_contour", poses, refined, trace, prm.damped.base.max_iterations,
            [&](const float* P, int n, float* Q, stocs_refine_visible_contour_result* r, stocs_refine_visible_trace* t) { return stocs_refine_poses_visible_contour(ctx_, P, n, &prm, Q, r, t); });
    }

    // Multi-instance selection (stocs_select_instances; no reference counterpart): which of the camera-frame hypotheses (the
    // hypotheses of run_trials, refined or not) are distinct instances of the object and which are one instance found twice.  Walked
    // best first, a hypothesis is kept only if enough of the scene points it explains are explained by none kept before it.  One record
    // per hypothesis in input order, and the indices of the kept ones in rank order in *selected.  The poses go to the centred frame in
    // float, as the tracking entry point brings its priors there: same linear part, t = (t_camera - c_scene) + R c_model.  Empty on
    // error (the text goes to the log).
    static stocs_instance_params default_instance_params() {
        stocs_instance_params p;
        stocs_default_instance_params(&p);
        return p;
    }
    std::vector<stocs_instance_result> select_instances(const std::vector<PoseCandidate*>& poses, std::vector<int>* selected,
                                                        const stocs_instance_params& prm = default_instance_params()) {
        const int n = (int)poses.size();
        float cs[3], cm[3];
        stocs_get_centroids(ctx_, cs, cm);
        std::vector<float> T((size_t)n * 16);
        for (int i = 0; i < n; ++i) {
            const float* P = poses[(size_t)i]->transform.data();
            float* dst = &T[(size_t)i * 16];
            bool zero = true;
            for (int k = 0; k < 16; ++k) zero = zero && P[k] == 0.0f;
            if (zero) { for (int k = 0; k < 16; ++k) dst[k] = 0.0f; continue; }   // a "no pose" record stays one
            for (int c = 0; c < 3; ++c) { for (int r = 0; r < 3; ++r) dst[c * 4 + r] = P[c * 4 + r]; dst[c * 4 + 3] = 0.0f; }
            for (int r = 0; r < 3; ++r) {
                const float rcm = P[r] * cm[0] + (P[4 + r] * cm[1] + P[8 + r] * cm[2]);
                dst[12 + r] = (P[12 + r] - cs[r]) + rcm;
            }
            dst[15] = 1.0f;
        }
        std::vector<stocs_instance_result> rec((size_t)n);
        std::vector<int32_t> sel((size_t)std::max(1, std::min(prm.max_instances, n)));
        int ns = 0;
        if (stocs_select_instances(ctx_, T.data(), n, &prm, rec.data(), sel.data(), &ns) != STOCS_OK) {
            *log_ << "select_instances failed: " << stocs_last_error() << std::endl;
            rec.clear(); ns = 0;
        }
        if (selected) selected->assign(sel.begin(), sel.begin() + ns);
        return rec;
    }

    // Scene-level selection across objects (stocs_scene_footprints; no reference counterpart): the pixels of the frame of set_frame that
    // each camera-frame hypothesis of THIS estimator's model claims -- claim 0: where the depth image agrees with it, 1: those of them on the
    // object's class mask -- written as bit rows into slots slot_base .. of a device pool that several estimators share (n_slots rows of
    // stocs_scene_row_words uint32_t each), and one record per hypothesis in input order.  stocs::select_scene below runs the whole step.
    // Empty on error (the text goes to the log).
    static stocs_scene_params default_scene_params() {
        stocs_scene_params p;
        stocs_default_scene_params(&p);
        return p;
    }
    std::vector<stocs_scene_record> scene_footprints(const std::vector<PoseCandidate*>& poses, void* d_rows, int slot_base, int n_slots, int claim = 0,
                                                     const stocs_render_params& prm = default_render_params()) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<stocs_scene_record> r((size_t)n);
        if (n > 0 && stocs_scene_footprints(ctx_, P.data(), n, slot_base, n_slots, &prm, claim, d_rows, r.data()) != STOCS_OK) {
            *log_ << "scene_footprints failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    // scene_footprints from the mesh of set_mesh (stocs_scene_footprints_mesh): the same rows and records; a pool may mix both kinds
    std::vector<stocs_scene_record> scene_footprints_mesh(const std::vector<PoseCandidate*>& poses, void* d_rows, int slot_base, int n_slots, int claim = 0,
                                                          const stocs_render_params& prm = default_render_params()) {
        const int n = (int)poses.size();
        std::vector<float> P((size_t)n * 16);
        for (int i = 0; i < n; ++i) std::memcpy(&P[(size_t)i * 16], poses[(size_t)i]->transform.data(), 64);
        std::vector<stocs_scene_record> r((size_t)n);
        if (n > 0 && stocs_scene_footprints_mesh(ctx_, P.data(), n, slot_base, n_slots, &prm, claim, d_rows, r.data()) != STOCS_OK) {
            *log_ << "scene_footprints_mesh failed: " << stocs_last_error() << std::endl;
            r.clear();
        }
        return r;
    }
    int frame_width() const { return image_width; }
    int frame_height() const { return image_height; }
    std::ostream& log() { return *log_; }

protected:
    std::vector<std::unique_ptr<PoseCandidate> > tracked_store_;   // results of the last track_poses
    std::unique_ptr<PoseCandidate> trial_best_;
    std::vector<std::unique_ptr<PoseCandidate> > refined_store_;   // results of the last refine_pose_candidates
    std::vector<std::unique_ptr<PoseCandidate> > hyp_store_;       // hypotheses of the last post-processed run_trials
    void reset_members(const std::string& dbg, int w, int h, float dist, int tr, int rot, float edge_thr, float class_thr) {
        ctx_ = NULL; log_ = &std::cout; best_lcp = 0; best_index = -1; seed_ = 0; attempt_ = 0; batched_ = false; fetched_ = false; n_batched_ = 0;
        la_n_ = 0; la_first_ = 0; la_seed_ = 0; la_cursor_ = 0; la_in_ctx_ = false; la_congruent_done_ = false; la_mode_ = 0; la_nvalid_ = 0;
        debug_location = dbg; image_width = w; image_height = h; distance_threshold = dist; ppf_tr_discretization = tr;
        ppf_rot_discretization = rot; edge_threshold = edge_thr; class_threshold = class_thr;
    }
    void ingest(const uint16_t* depth, const uint16_t* prob, const uint8_t* edge, const std::vector<float>& K, float read_depth_scale, float write_depth_scale,
                float voxel_size, const std::string& dst_scene_location) {
        if (K.size() < 4) throw std::runtime_error("camera_intrinsics must hold {fx, cx, fy, cy}");
        stocs_camera cam;
        cam.fx = K[0]; cam.cx = K[1]; cam.fy = K[2]; cam.cy = K[3]; cam.depth_scale = read_depth_scale; cam.width = image_width; cam.height = image_height;
        cam.normal_method = STOCS_NORMALS_DEPTH_GRADIENT;   // rgbd.cpp:203: RGBD_NORMALS_METHOD_LINEMOD
        const int cap = image_width * image_height;
        scene_.pos.resize((size_t)cap * 3); scene_.nrm.resize((size_t)cap * 3); scene_.class_probability.resize((size_t)cap); scene_.pixel.resize((size_t)cap * 2);
        int n = 0;
        if (stocs_ingest_scene(&cam, depth, prob, voxel_size, class_threshold, -1, scene_.pos.data(), scene_.nrm.data(), scene_.class_probability.data(),
                               scene_.pixel.data(), cap, &n) != STOCS_OK)
            throw std::runtime_error(std::string("stocs_ingest_scene: ") + stocs_last_error());
        scene_.pos.resize((size_t)n * 3); scene_.nrm.resize((size_t)n * 3); scene_.class_probability.resize((size_t)n); scene_.pixel.resize((size_t)n * 2);
        scene_.edge_map.clear();
        if (edge) scene_.edge_map.assign(edge, edge + (size_t)cap);
        if (!dst_scene_location.empty())   // rgbd::save_as_ply(dst_scene_location, point3d_scene, write_depth_scale), stocs.cpp:130
            (void)stocs_ply_write(dst_scene_location.c_str(), scene_.pos.data(), scene_.nrm.data(), n, write_depth_scale);
    }
    void create_context(int device) {
        stocs_default_params(&prm_);
        prm_.distance_threshold = distance_threshold;
        prm_.ppf_tr_discretization = ppf_tr_discretization;
        prm_.ppf_rot_discretization = ppf_rot_discretization;
        prm_.image_width = image_width;
        prm_.image_height = image_height;
        const bool load = !ppf_location_.empty();
        int rc = stocs_ctx_create(&prm_, scene_.pos.data(), scene_.nrm.data(), scene_.class_probability.data(), scene_.pixel.empty() ? NULL : scene_.pixel.data(),
                                  scene_.size(), model_.pos.data(), model_.nrm.data(), model_.size(), load ? 0 : 1, device, &ctx_);
        if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_ctx_create: ") + stocs_last_error());
        if (load && (rc = stocs_index_load(ctx_, ppf_location_.c_str())) != STOCS_OK) {
            const std::string msg = std::string("stocs_index_load: ") + stocs_last_error();
            stocs_ctx_destroy(ctx_); ctx_ = NULL;
            throw std::runtime_error(msg);
        }
        if (!scene_.edge_map.empty()) stocs_set_edge_map(ctx_, scene_.edge_map.data());
        *log_ << "|S|: " << scene_.size() << std::endl;   // stocs.cpp:970
    }
    // One attempt of the reference's one-per-call loop.  Class mode: the attempts do not depend on each other (every base
    // starts from the prior, stocs.cpp:372-381; attempt a is seeded by (seed, a)), so the facade draws a block of them in one
    // GPU pass and serves the calls from the block -- the results are those of one call per attempt.  Instance mode is
    // sequential state (and decays the class probabilities the LCP reads, Q8): one attempt per call, nothing ahead of the caller.
    bool sample_one(int mode, float dispersion, std::vector<int>& base_indices, float& invariant1, float& invariant2) {
        int32_t ids[4] = {-1, -1, -1, -1};
        float inv[2] = {0, 0};
        int32_t valid = 0;
        if (mode == 0) {
            if (!(la_mode_ == 0 && la_n_ > 0 && la_seed_ == seed_ && attempt_ >= la_first_ && attempt_ < la_first_ + la_n_)) {
                la_n_ = 0; la_in_ctx_ = false; la_congruent_done_ = false;
                la_ids_.assign((size_t)kLookahead * 4, -1); la_inv_.assign((size_t)kLookahead * 2, 0.0f); la_valid_.assign((size_t)kLookahead, 0);
                if (stocs_clear_bases(ctx_) != STOCS_OK ||
                    stocs_sample_bases(ctx_, 0, seed_, attempt_, kLookahead, 0.0f, la_ids_.data(), la_inv_.data(), la_valid_.data()) != STOCS_OK)
                    return false;
                la_first_ = attempt_; la_n_ = kLookahead; la_seed_ = seed_; la_in_ctx_ = true; la_cursor_ = 0; la_mode_ = 0;
                la_slot_of_.assign((size_t)kLookahead, -1);                  // base slot in the context of every valid attempt
                int slot = 0;
                for (int k = 0; k < kLookahead; ++k) if (la_valid_[(size_t)k]) la_slot_of_[(size_t)k] = slot++;
            }
            const size_t k = (size_t)(attempt_ - la_first_);
            for (int j = 0; j < 4; ++j) ids[j] = la_ids_[4 * k + (size_t)j];
            inv[0] = la_inv_[2 * k]; inv[1] = la_inv_[2 * k + 1];
            valid = la_valid_[k];
            ++attempt_;
        } else {
            // nothing is drawn ahead; but the context keeps the valid bases in attempt order, so the facade remembers which
            // slot each one got -- find_congruent_sets_on_model then searches once for all of them
            if (attempt_ == 0 || la_mode_ != 1) {
                la_ids_.clear(); la_inv_.clear(); la_valid_.clear(); la_slot_of_.clear();
                la_n_ = 0; la_nvalid_ = 0; la_cursor_ = 0; la_mode_ = 1;
                la_in_ctx_ = stocs_clear_bases(ctx_) == STOCS_OK;
            }
            if (stocs_sample_bases(ctx_, mode, seed_, attempt_++, 1, dispersion, ids, inv, &valid) != STOCS_OK) { la_in_ctx_ = false; return false; }
            la_ids_.insert(la_ids_.end(), ids, ids + 4); la_inv_.insert(la_inv_.end(), inv, inv + 2); la_valid_.push_back(valid);
            la_slot_of_.push_back(valid ? la_nvalid_++ : -1);
            ++la_n_;
            la_congruent_done_ = false;                                      // the base set grew: an earlier search does not cover it
        }
        if (base_indices.size() < 4) base_indices.resize(4);
        for (int k = 0; k < 4; ++k) base_indices[(size_t)k] = ids[k];
        invariant1 = inv[0];
        invariant2 = inv[1];
        return valid != 0;
    }
    // slot in the context's base set of a base the look-ahead block sampled (so that its congruent sets come out of ONE
    // search over all the block's bases), or -1
    int lookahead_slot(const int32_t* ids, const float* inv) {
        if (!la_in_ctx_ || la_n_ <= 0) return -1;
        for (int step = 0; step < la_n_; ++step) {                           // the caller walks the bases in order: found at the cursor
            const size_t k = (size_t)((la_cursor_ + step) % la_n_);
            if (la_slot_of_[k] < 0) continue;
            if (std::memcmp(&la_ids_[4 * k], ids, 16) == 0 && std::memcmp(&la_inv_[2 * k], inv, 8) == 0) { la_cursor_ = (int)k; return la_slot_of_[k]; }
        }
        return -1;
    }
    // candidates of make_transforms -> all_transforms / all_pose, on demand
    void fetch_batched() {
        if (!batched_ || fetched_) return;
        int n = 0;
        stocs_get_candidates(ctx_, NULL, NULL, NULL, NULL, 0, &n);
        std::vector<float> T((size_t)n * 16), P((size_t)n * 16), l((size_t)n);
        std::vector<int32_t> b((size_t)n);
        if (n) stocs_get_candidates(ctx_, T.data(), P.data(), l.data(), b.data(), n, &n);
        all_transforms.assign((size_t)n, Mat4f()); all_pose.clear(); all_pose_store_.clear();
        for (int i = 0; i < n; ++i) {
            std::memcpy(all_transforms[(size_t)i].data(), &T[(size_t)i * 16], 64);
            Mat4f pm; std::memcpy(pm.data(), &P[(size_t)i * 16], 64);
            all_pose_store_.emplace_back(new PoseCandidate(pm, l[(size_t)i], (float)b[(size_t)i]));
            all_pose.push_back(all_pose_store_.back().get());
        }
        fetched_ = true;
    }
    // the estimator's clouds as the reference holds them after centroid_shift (stocs.cpp:943-964)
    std::vector<Point3D> scene_points() {
        const int n = scene_.size();
        std::vector<float> p((size_t)n * 3), nr((size_t)n * 3), pr((size_t)n);
        std::vector<int32_t> px((size_t)n * 2);
        stocs_get_scene(ctx_, p.data(), nr.data(), pr.data(), px.data());
        std::vector<Point3D> out;
        out.reserve((size_t)n);
        for (int i = 0; i < n; ++i) {
            Point3D q(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
            q.set_normal(VectorType(nr[3 * i], nr[3 * i + 1], nr[3 * i + 2]));
            q.set_pixel(std::make_pair((int)px[2 * i], (int)px[2 * i + 1]));
            const float e = scene_.edge_map.empty() ? 0.0f : (float)(255.0 - scene_.edge_map[(size_t)px[2 * i] * image_width + px[2 * i + 1]]) / 255.0f;
            q.set_probability(pr[i], e);
            out.push_back(q);
        }
        return out;
    }
    std::vector<Point3D> model_points_centred() {
        float cm[3] = {0, 0, 0};
        stocs_get_centroids(ctx_, NULL, cm);
        std::vector<Point3D> out;
        for (int i = 0; i < model_.size(); ++i) {
            Point3D q(model_.pos[3 * i] - cm[0], model_.pos[3 * i + 1] - cm[1], model_.pos[3 * i + 2] - cm[2]);
            q.set_normal(VectorType(model_.nrm[3 * i], model_.nrm[3 * i + 1], model_.nrm[3 * i + 2]));
            out.push_back(q);
        }
        return out;
    }

    stocs_ctx* ctx_;
    std::ostream* log_;
    stocs_params prm_;
    ModelCloud model_;
    SceneCloud scene_;
    std::string ppf_location_;
    std::vector<MatrixType> all_transforms;
    std::vector<PoseCandidate*> all_pose;
    std::vector<std::unique_ptr<PoseCandidate> > all_pose_store_;
    std::vector<int32_t> base_ids_, base_valid_;
    std::vector<float> base_inv_;
    std::string debug_location;
    float distance_threshold;
    int ppf_tr_discretization, ppf_rot_discretization;
    float edge_threshold, class_threshold;
    Scalar best_lcp;
    int best_index;
    int image_width, image_height;
    uint64_t seed_;
    int attempt_;
    bool batched_, fetched_;
    int n_batched_;
    // look-ahead block of class-mode attempts / the instance-mode attempts made so far (sample_one)
    enum { kLookahead = 100 };           // the reference's number_of_bases (stocs_match_one_object.cpp:16)
    std::vector<int32_t> la_ids_, la_valid_;
    std::vector<float> la_inv_;
    std::vector<int> la_slot_of_;
    uint64_t la_seed_;
    int la_first_, la_n_, la_cursor_, la_mode_, la_nvalid_;
    bool la_in_ctx_, la_congruent_done_;
};

// Not in the reference: the symmetry transforms that a clustering descriptor (0, 90, 180 or 360 per axis, the reference's sym_info) stands
// for (stocs_symmetry_set): K x 16 floats, column-major, entry 0 the identity; a continuous axis is sampled at n_continuous steps, the
// rotations turn about center3 (NULL: the origin).  Empty on error.
inline std::vector<float> symmetry_set(const float sym3[3], int n_continuous = 72, const float* center3 = NULL) {
    int K = 0;
    (void)stocs_symmetry_set(sym3, n_continuous, center3, NULL, 0, &K);   // the count alone: no room is offered
    std::vector<float> out((size_t)(K > 0 ? K : 0) * 16);
    if (K < 1 || stocs_symmetry_set(sym3, n_continuous, center3, out.data(), K, &K) != STOCS_OK) out.clear();
    return out;
}

// Not in the reference: the closure of generators (n x 16 floats, column-major) under composition (stocs_symmetry_close): K x 16 floats,
// entry 0 the identity; *truncated (when given) says that the closure stopped at cap.  Empty on error.
inline std::vector<float> symmetry_close(const std::vector<float>& gen16, float same_deg = 1.25f, int cap = STOCS_POSE_SYM_MAX, bool* truncated = NULL) {
    std::vector<float> out((size_t)(cap > 0 ? cap : 0) * 16);
    int K = 0, tr = 0;
    if (stocs_symmetry_close(gen16.data(), (int)(gen16.size() / 16), same_deg, out.data(), cap, &K, &tr) != STOCS_OK) K = 0;
    out.resize((size_t)K * 16);
    if (truncated) *truncated = tr != 0;
    return out;
}

// Not in the reference: the symmetries of a sampled model file (model_search.ply, as pre_process_model writes it) without a scene: a
// context on the model alone (a one-point scene, no index), then stocs_find_symmetries.  Throws when the file or the context fails.
inline SymmetryResult find_model_symmetries(const std::string& model_location, const stocs_symmetry_search& search = default_symmetry_search()) {
    ModelCloud m;
    read_ply(model_location, &m, true);
    const float sp[3] = {0, 0, 1}, sn[3] = {0, 0, -1}, spr[1] = {1.0f};
    stocs_params prm;
    stocs_default_params(&prm);
    stocs_ctx* ctx = NULL;
    if (stocs_ctx_create(&prm, sp, sn, spr, NULL, 1, m.pos.data(), m.nrm.data(), m.size(), 0, -1, &ctx) != STOCS_OK)
        throw std::runtime_error(std::string("stocs_ctx_create: ") + stocs_last_error());
    SymmetryResult r = find_symmetries_of(ctx, search, NULL);
    const std::string msg = r.ok ? std::string() : std::string("stocs_find_symmetries: ") + stocs_last_error();
    stocs_ctx_destroy(ctx);
    if (!r.ok) throw std::runtime_error(msg);
    return r;
}

// Not in the reference: which hypotheses of several objects form one consistent explanation of the frame (stocs_scene_footprints /
// stocs_scene_select).  estimators[k] holds object k's model and the frame (set_frame, the same size everywhere), poses[k] its camera-frame
// hypotheses.  The pool of pixel rows is allocated on the first estimator's device, every estimator writes its footprints into
// consecutive slots (group = object index), and the first estimator walks the pool.  The score of a slot is float(agree) /
// float(footprint), 0 where the footprint is empty: visible-surface agreement, comparable across objects.  max_per_object: empty (no
// cap), one cap for all, or one per object.  with_labels: the selected poses are rendered into one key buffer with id = slot
// (stocs_render_poses) and labels / state come from stocs_render_labels of the first estimator.  ok == false on error (the text goes to
// the first estimator's log).
struct SceneSelection {
    bool ok;
    std::vector<int32_t> group, index;             // per slot: the object and the hypothesis of it
    std::vector<float> score;
    std::vector<stocs_scene_record> footprints;
    std::vector<stocs_scene_result> records;
    std::vector<int> selected;                     // slots in rank order
    std::vector<int32_t> labels;                   // with_labels: -1 or the slot that owns the pixel
    std::vector<uint8_t> state;
};
// The surface an object's footprints and masks are taken from: its model points as splats, or the mesh of its estimator's set_mesh
enum SceneSurface { SURFACE_POINTS = 0, SURFACE_MESH = 1 };
// ... with a surface per object (empty: all points): a SURFACE_MESH object goes through scene_footprints_mesh and, with_labels,
// stocs_render_poses_mesh; both kinds share the pool and the key buffer
inline SceneSelection select_scene(const std::vector<stocs_estimator*>& estimators, const std::vector<std::vector<PoseCandidate*> >& poses,
                                   const std::vector<SceneSurface>& surface, const std::vector<int>& max_per_object = std::vector<int>(), bool with_labels = false,
                                   const stocs_scene_params& prm = stocs_estimator::default_scene_params(),
                                   const stocs_render_params& render = stocs_estimator::default_render_params(), int claim = 0) {
    SceneSelection out;
    out.ok = false;
    if (estimators.empty() || estimators.size() != poses.size()) throw std::runtime_error("select_scene: one pose set per estimator");
    if (!surface.empty() && surface.size() != estimators.size()) throw std::runtime_error("select_scene: one surface per object");
    if (!max_per_object.empty() && max_per_object.size() != 1 && max_per_object.size() != estimators.size()) throw std::runtime_error("select_scene: one cap, or one per object");
    stocs_estimator& first = *estimators[0];
    const int W = first.frame_width(), H = first.frame_height();
    int n = 0;
    for (size_t k = 0; k < poses.size(); ++k) {
        if (estimators[k]->frame_width() != W || estimators[k]->frame_height() != H) throw std::runtime_error("select_scene: the estimators' frames differ in size");
        for (size_t i = 0; i < poses[k].size(); ++i) { out.group.push_back((int32_t)k); out.index.push_back((int32_t)i); }
        n += (int)poses[k].size();
    }
    const int Wr = stocs_scene_row_words(W, H);
    void* d_rows = NULL;
    void* d_zkey = NULL;
    if (stocs_dev_alloc(first.context(), (int64_t)std::max(n, 1) * Wr * 4, &d_rows) != STOCS_OK) { first.log() << "select_scene failed: " << stocs_last_error() << std::endl; return out; }
    bool good = true;
    int base = 0;
    for (size_t k = 0; good && k < poses.size(); ++k) {
        const bool mesh = !surface.empty() && surface[k] == SURFACE_MESH;
        const std::vector<stocs_scene_record> r = mesh ? estimators[k]->scene_footprints_mesh(poses[k], d_rows, base, n, claim, render)
                                                       : estimators[k]->scene_footprints(poses[k], d_rows, base, n, claim, render);
        good = r.size() == poses[k].size();
        out.footprints.insert(out.footprints.end(), r.begin(), r.end());
        base += (int)poses[k].size();
    }
    if (good) {
        out.score.resize((size_t)n);
        for (int h = 0; h < n; ++h) out.score[(size_t)h] = out.footprints[(size_t)h].footprint > 0 ? (float)out.footprints[(size_t)h].agree / (float)out.footprints[(size_t)h].footprint : 0.0f;
        std::vector<int32_t> cap;
        for (size_t k = 0; !max_per_object.empty() && k < estimators.size(); ++k) cap.push_back(max_per_object[max_per_object.size() == 1 ? 0 : k]);
        out.records.resize((size_t)n);
        std::vector<int32_t> sel((size_t)std::max(n, 1));
        int ns = 0;
        good = stocs_scene_select(first.context(), d_rows, n, W, H, out.score.data(), out.group.data(), out.footprints.data(), (int)estimators.size(),
                                  cap.empty() ? NULL : cap.data(), &prm, out.records.data(), sel.data(), &ns) == STOCS_OK;
        if (good) out.selected.assign(sel.begin(), sel.begin() + ns);
    }
    if (good && with_labels) {
        const size_t npix = (size_t)W * (size_t)H;
        out.labels.assign(npix, -1);
        out.state.assign(npix, 0);
        if (!out.selected.empty()) {
            good = stocs_dev_alloc(first.context(), (int64_t)npix * 8, &d_zkey) == STOCS_OK;
            for (size_t r = 0; good && r < out.selected.size(); ++r) {
                const int s = out.selected[r];
                PoseCandidate* pc = poses[(size_t)out.group[(size_t)s]][(size_t)out.index[(size_t)s]];
                const size_t g = (size_t)out.group[(size_t)s];
                good = (!surface.empty() && surface[g] == SURFACE_MESH
                            ? stocs_render_poses_mesh(estimators[g]->context(), pc->transform.data(), 1, s, d_zkey, r == 0 ? 1 : 0)
                            : stocs_render_poses(estimators[g]->context(), pc->transform.data(), 1, s, &render, d_zkey, r == 0 ? 1 : 0)) == STOCS_OK;
            }
            good = good && stocs_render_labels(first.context(), d_zkey, &render, out.labels.data(), out.state.data()) == STOCS_OK;
        }
    }
    if (!good) first.log() << "select_scene failed: " << stocs_last_error() << std::endl;
    if (d_zkey) stocs_dev_free(first.context(), d_zkey);
    stocs_dev_free(first.context(), d_rows);
    out.ok = good;
    return out;
}
inline SceneSelection select_scene(const std::vector<stocs_estimator*>& estimators, const std::vector<std::vector<PoseCandidate*> >& poses,
                                   const std::vector<int>& max_per_object = std::vector<int>(), bool with_labels = false,
                                   const stocs_scene_params& prm = stocs_estimator::default_scene_params(),
                                   const stocs_render_params& render = stocs_estimator::default_render_params(), int claim = 0) {
    return select_scene(estimators, poses, std::vector<SceneSurface>(), max_per_object, with_labels, prm, render, claim);
}

// Not in the reference (its class and edge images come from a network): both from the depth image alone (stocs_segment_frame) -- the
// support plane removed, what stands on it split into depth-connected segments.  class_prob is what the estimator's image constructor
// and set_frame take, edge what they take as the edge map (255 = interior), labels the segment numbers 1 .. records.size().
struct SegmentedFrame {
    stocs_segment_result result;
    std::vector<stocs_segment_record> records;
    std::vector<uint16_t> class_prob;
    std::vector<int32_t> labels;
    std::vector<uint8_t> edge;
    stocs_segment_convex_result convex;   // the concavity cut's counts; zero from the overload without it
    std::vector<uint8_t> cut;             // from the overload with the cut: bit 0 horizontal, bit 1 vertical
};
inline stocs_segment_params default_segment_params() { stocs_segment_params p; stocs_default_segment_params(&p); return p; }
inline stocs_segment_convex_params default_segment_convex_params() { stocs_segment_convex_params p; stocs_default_segment_convex_params(&p); return p; }
// both overloads below: the camera, the vectors sized, the call (convex NULL: stocs_segment_frame, and out.convex stays zero), the throw
inline SegmentedFrame segment_frame_impl(const uint16_t* depth, const std::vector<float>& camera_intrinsics, int image_width, int image_height, float read_depth_scale,
                                         const stocs_segment_params& prm, const stocs_segment_convex_params* convex, int device) {
    if (camera_intrinsics.size() < 4) throw std::runtime_error("camera_intrinsics must hold {fx, cx, fy, cy}");
    if (image_width < 1 || image_height < 1 || prm.min_pixels < 1) throw std::runtime_error("segment_frame: an empty frame or min_pixels < 1");
    stocs_camera cam;
    cam.fx = camera_intrinsics[0]; cam.cx = camera_intrinsics[1]; cam.fy = camera_intrinsics[2]; cam.cy = camera_intrinsics[3];
    cam.depth_scale = read_depth_scale; cam.width = image_width; cam.height = image_height;
    cam.normal_method = STOCS_NORMALS_DEPTH_GRADIENT;   // (not looked at)
    SegmentedFrame out;
    memset(&out.convex, 0, sizeof(out.convex));
    const size_t npix = (size_t)image_width * image_height, cap = npix / (size_t)prm.min_pixels;   // no more segments than this fit the frame
    out.records.resize(cap ? cap : 1);
    out.class_prob.resize(npix); out.labels.resize(npix); out.edge.resize(npix);
    if (convex) out.cut.resize(npix);
    const int rc = convex ? stocs_segment_frame_convex(&cam, depth, &prm, convex, device, out.class_prob.data(), out.labels.data(), out.edge.data(), out.cut.data(), NULL, out.records.data(),
                                                       (int)cap, &out.result, &out.convex)
                          : stocs_segment_frame(&cam, depth, &prm, device, out.class_prob.data(), out.labels.data(), out.edge.data(), out.records.data(), (int)cap, &out.result);
    if (rc != STOCS_OK) throw std::runtime_error(std::string(convex ? "stocs_segment_frame_convex: " : "stocs_segment_frame: ") + stocs_last_error());
    out.records.resize((size_t)out.result.n_segments);
    return out;
}
inline SegmentedFrame segment_frame(const uint16_t* depth, const std::vector<float>& camera_intrinsics, int image_width, int image_height, float read_depth_scale,
                                    const stocs_segment_params& prm = default_segment_params(), int device = -1) {
    return segment_frame_impl(depth, camera_intrinsics, image_width, image_height, read_depth_scale, prm, NULL, device);
}
// The same with the concavity cut in front of the labelling (stocs_segment_frame_convex): touching objects come apart at concave creases.
inline SegmentedFrame segment_frame(const uint16_t* depth, const std::vector<float>& camera_intrinsics, int image_width, int image_height, float read_depth_scale,
                                    const stocs_segment_params& prm, const stocs_segment_convex_params& convex, int device = -1) {
    return segment_frame_impl(depth, camera_intrinsics, image_width, image_height, read_depth_scale, prm, &convex, device);
}

// Not in the reference: the join between the segments of a frame and the objects with models (stocs_segment_shapes, stocs_segment_assign).
// A label image (segment_frame's or anybody's, 1 .. n_labels) -> one 3-D shape per label; with objects, the size gate's reason bits
// (reasons[k * n_labels + l]: object k, label l + 1; 0 = compatible) and the object-major class stack load_frame_scenes takes.  The
// gate is not exclusive: objects of like size keep the same segments, and choosing among them is select_scene's job.
struct SegmentAssignment {
    stocs_segment_shapes_result result;
    std::vector<stocs_segment_shape> shapes;   // n_labels
    std::vector<uint8_t> reasons;              // n_objects x n_labels, STOCS_GATE_* bits
    std::vector<uint16_t> class_stack;         // n_objects x image_height x image_width: 10000 where the pixel's label is compatible
    int n_labels, n_objects;
    int compatible(int object) const {         // the segments the gate leaves the object
        int c = 0;
        for (int l = 0; l < n_labels; ++l) c += reasons[(size_t)object * n_labels + l] == 0 ? 1 : 0;
        return c;
    }
};
inline stocs_segment_gate_params default_segment_gate_params() { stocs_segment_gate_params g; stocs_default_segment_gate_params(&g); return g; }
// an object's size from its (preprocessed) model cloud: the extents of stocs_points_shape; the diameter is the caller's exact one or,
// with diameter <= 0, the diagonal of the extents formed in double and cast once: an upper bound, so TOO_LARGE stays sound
inline stocs_object_size object_size(const std::vector<float>& model_pos, float diameter = 0.0f, int device = -1) {
    stocs_segment_shape s;
    if (stocs_points_shape(model_pos.data(), (int)(model_pos.size() / 3), device, &s, NULL) != STOCS_OK) throw std::runtime_error(std::string("stocs_points_shape: ") + stocs_last_error());
    stocs_object_size o;
    for (int k = 0; k < 3; ++k) o.extent[k] = s.extent[k];
    o.diameter = diameter > 0.0f ? diameter
                                 : (float)std::sqrt((double)s.extent[0] * (double)s.extent[0] + ((double)s.extent[1] * (double)s.extent[1] + (double)s.extent[2] * (double)s.extent[2]));
    return o;
}
inline SegmentAssignment segment_assign(const uint16_t* depth, const int32_t* labels, int n_labels, const std::vector<stocs_object_size>& objects,
                                        const std::vector<float>& camera_intrinsics, int image_width, int image_height, float read_depth_scale, float max_depth = 2.0f,
                                        const stocs_segment_gate_params& gate = default_segment_gate_params(), int device = -1) {
    if (camera_intrinsics.size() < 4) throw std::runtime_error("camera_intrinsics must hold {fx, cx, fy, cy}");
    if (image_width < 1 || image_height < 1 || n_labels < 0) throw std::runtime_error("segment_assign: an empty frame or n_labels < 0");
    stocs_camera cam;
    cam.fx = camera_intrinsics[0]; cam.cx = camera_intrinsics[1]; cam.fy = camera_intrinsics[2]; cam.cy = camera_intrinsics[3];
    cam.depth_scale = read_depth_scale; cam.width = image_width; cam.height = image_height;
    cam.normal_method = STOCS_NORMALS_DEPTH_GRADIENT;   // (not looked at)
    SegmentAssignment out;
    out.n_labels = n_labels; out.n_objects = (int)objects.size();
    out.shapes.resize((size_t)n_labels);
    out.reasons.resize(objects.size() * (size_t)n_labels);
    out.class_stack.resize(objects.size() * (size_t)image_width * image_height);
    const int rc = stocs_segment_assign(&cam, depth, labels, n_labels, max_depth, objects.empty() ? NULL : objects.data(), out.n_objects, &gate, device,
                                        n_labels ? out.shapes.data() : NULL, NULL, out.reasons.empty() ? NULL : out.reasons.data(),
                                        objects.empty() ? NULL : out.class_stack.data(), &out.result);
    if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_segment_assign: ") + stocs_last_error());
    return out;
}
inline SegmentAssignment segment_shapes(const uint16_t* depth, const int32_t* labels, int n_labels, const std::vector<float>& camera_intrinsics, int image_width,
                                        int image_height, float read_depth_scale, float max_depth = 2.0f, int device = -1) {
    return segment_assign(depth, labels, n_labels, std::vector<stocs_object_size>(), camera_intrinsics, image_width, image_height, read_depth_scale, max_depth,
                          default_segment_gate_params(), device);
}

// Not in the reference (its driver runs once per object): every object of one frame from one ingest (stocs_ingest_scene_multi).
// class_probability_maps holds class_thresholds.size() images of image_height x image_width, object after object; edge (may be NULL)
// is shared by all of them.  Scene k is what the estimator's own ingest makes of (depth, map k, class_thresholds[k]), bit for bit.
inline std::vector<SceneCloud> load_frame_scenes(const uint16_t* depth, const uint16_t* class_probability_maps, const std::vector<float>& class_thresholds,
                                                 const uint8_t* edge, const std::vector<float>& camera_intrinsics, int image_width, int image_height,
                                                 float read_depth_scale, float voxel_size, int device = -1) {
    if (camera_intrinsics.size() < 4) throw std::runtime_error("camera_intrinsics must hold {fx, cx, fy, cy}");
    stocs_camera cam;
    cam.fx = camera_intrinsics[0]; cam.cx = camera_intrinsics[1]; cam.fy = camera_intrinsics[2]; cam.cy = camera_intrinsics[3];
    cam.depth_scale = read_depth_scale; cam.width = image_width; cam.height = image_height;
    cam.normal_method = STOCS_NORMALS_DEPTH_GRADIENT;   // as stocs_estimator::ingest
    const int n_obj = (int)class_thresholds.size();
    std::vector<int32_t> off((size_t)n_obj + 1, 0);
    std::vector<float> pos, nrm, prob;
    std::vector<int32_t> pix;
    int cap = image_width * image_height;   // one frame's worth of points; grown once when the objects need more
    for (int pass = 0; pass < 2; ++pass) {
        pos.resize((size_t)cap * 3); nrm.resize((size_t)cap * 3); prob.resize((size_t)cap); pix.resize((size_t)cap * 2);
        const int rc = stocs_ingest_scene_multi(&cam, depth, n_obj, class_probability_maps, class_thresholds.data(), voxel_size, device, pos.data(), nrm.data(),
                                                prob.data(), pix.data(), cap, off.data());
        if (rc == STOCS_ERR_CAPACITY && pass == 0) { cap = off[(size_t)n_obj]; continue; }
        if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_ingest_scene_multi: ") + stocs_last_error());
        break;
    }
    std::vector<SceneCloud> out((size_t)n_obj);
    for (int k = 0; k < n_obj; ++k) {
        SceneCloud& sc = out[(size_t)k];
        const size_t a = (size_t)off[(size_t)k], b = (size_t)off[(size_t)k + 1];
        sc.pos.assign(pos.begin() + 3 * a, pos.begin() + 3 * b); sc.nrm.assign(nrm.begin() + 3 * a, nrm.begin() + 3 * b);
        sc.class_probability.assign(prob.begin() + a, prob.begin() + b); sc.pixel.assign(pix.begin() + 2 * a, pix.begin() + 2 * b);
        if (edge) sc.edge_map.assign(edge, edge + (size_t)image_width * image_height);
    }
    return out;
}
// the same from the reference's files: depth.png, one probability map per object, edge.png when it exists (as load_scene_info)
inline std::vector<SceneCloud> load_frame_scenes(std::string depth_location, const std::vector<std::string>& class_probability_map_locations,
                                                 const std::vector<float>& class_thresholds, std::string edge_probability_map_location,
                                                 const std::vector<float>& camera_intrinsics, int image_width, int image_height, float read_depth_scale,
                                                 float voxel_size, int device = -1) {
    if (class_probability_map_locations.size() != class_thresholds.size()) throw std::runtime_error("load_frame_scenes: one class threshold per probability map");
    std::vector<uint16_t> depth, maps, one;
    std::vector<uint8_t> edge;
    read_image(depth_location, 1, 16, image_width, image_height, &depth);
    for (size_t k = 0; k < class_probability_map_locations.size(); ++k) {
        read_image(class_probability_map_locations[k], 1, 16, image_width, image_height, &one);
        maps.insert(maps.end(), one.begin(), one.end());
    }
    const bool has_edge = file_exists(edge_probability_map_location);
    if (has_edge) read_image(edge_probability_map_location, 1, 8, image_width, image_height, &edge);
    return load_frame_scenes(depth.data(), maps.data(), class_thresholds, has_edge ? edge.data() : NULL, camera_intrinsics, image_width, image_height,
                             read_depth_scale, voxel_size, device);
}

// The file and index half of model preprocessing: the sampled cloud (n points) -> the model_search PLY + the PPF index of the cloud as
// the estimator will read it back (the written file), so the two always agree bit for bit.
inline void write_model_and_index(const ModelCloud& sampled, int n, float write_depth_scale, float ppf_tr_discretization, float ppf_rot_discretization,
                                  const std::string& dst_model_location, const std::string& dst_ppf_map_location) {
    std::cout << "After sampling |M|= " << n << std::endl;
    if (stocs_ply_write(dst_model_location.c_str(), sampled.pos.data(), sampled.nrm.data(), n, write_depth_scale) != STOCS_OK)
        throw std::runtime_error(std::string("stocs_ply_write: ") + stocs_last_error());
    ModelCloud written;
    read_ply(dst_model_location, &written, true);
    float max_distance = 0;   // "max distance is" (stocs.cpp:66-78), from the bounding box instead of the O(|M|^2) loop
    {
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
        for (int i = 0; i < written.size(); ++i)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], written.pos[3 * i + k]); hi[k] = std::max(hi[k], written.pos[3 * i + k]); }
        if (written.size()) max_distance = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    }
    std::cout << "max distance is at most: " << max_distance << std::endl;
    // a one-point scene is enough to own a context; the index depends on the model alone
    const float sp[3] = {0, 0, 1}, sn[3] = {0, 0, -1}, spr[1] = {1.0f};
    stocs_params prm;
    stocs_default_params(&prm);
    prm.ppf_tr_discretization = (int)ppf_tr_discretization;
    prm.ppf_rot_discretization = (int)ppf_rot_discretization;
    stocs_ctx* ctx = NULL;
    if (stocs_ctx_create(&prm, sp, sn, spr, NULL, 1, written.pos.data(), written.nrm.data(), written.size(), 1, -1, &ctx) != STOCS_OK)
        throw std::runtime_error(std::string("stocs_ctx_create: ") + stocs_last_error());
    const int rc = stocs_index_save(ctx, dst_ppf_map_location.c_str());
    const std::string msg = rc == STOCS_OK ? std::string() : std::string("stocs_index_save: ") + stocs_last_error();
    stocs_ctx_destroy(ctx);
    if (rc != STOCS_OK) throw std::runtime_error(msg);
}

// reference stocs.hpp:182-191 / stocs.cpp:28-84: raw model PLY -> normals (radius), flipped, voxel grid, scale -> model_search
// PLY + the PPF index of the sampled cloud, both on the GPU.
inline void pre_process_model(std::string src_model_location, float normal_radius, float read_depth_scale, float write_depth_scale, float voxel_size,
                              float ppf_tr_discretization, float ppf_rot_discretization, std::string dst_model_location, std::string dst_ppf_map_location) {
    ModelCloud raw, sampled;
    read_ply(src_model_location, &raw, false);
    sampled.pos.resize(raw.pos.size()); sampled.nrm.resize(raw.pos.size());
    int n = 0;
    if (stocs_preprocess_model(raw.pos.data(), raw.size(), normal_radius, voxel_size, read_depth_scale, -1, sampled.pos.data(), sampled.nrm.data(), raw.size(), &n) != STOCS_OK)
        throw std::runtime_error(std::string("stocs_preprocess_model: ") + stocs_last_error());
    write_model_and_index(sampled, n, write_depth_scale, ppf_tr_discretization, ppf_rot_discretization, dst_model_location, dst_ppf_map_location);
}

// Not in the reference: pre_process_model with the cloud stage exchanged: a triangle mesh (PLY with faces) is sampled on the GPU at one point
// per spacing^2 of area (0: voxel_size / 4), every normal its facet's (orient 0: the winding's, 1: turned away from the origin), then voxel
// grid and scale as above (stocs_preprocess_model_mesh).  A file without a readable mesh, or without faces, is refused.
inline void pre_process_model_mesh(std::string mesh_location, float spacing, uint64_t seed, int orient, float read_depth_scale, float write_depth_scale, float voxel_size,
                                   float ppf_tr_discretization, float ppf_rot_discretization, std::string dst_model_location, std::string dst_ppf_map_location) {
    int nv = 0, nt = 0;
    if (stocs_ply_read_mesh(mesh_location.c_str(), NULL, 0, &nv, NULL, 0, &nt) != STOCS_OK)
        throw std::runtime_error("cannot read a mesh from " + mesh_location + ": " + stocs_last_error());
    if (nt < 1) throw std::runtime_error(mesh_location + " has no faces");
    std::vector<float> mesh_v((size_t)nv * 3);
    std::vector<int32_t> mesh_t((size_t)nt * 3);
    if (stocs_ply_read_mesh(mesh_location.c_str(), mesh_v.data(), nv, &nv, mesh_t.data(), nt, &nt) != STOCS_OK)
        throw std::runtime_error("cannot read a mesh from " + mesh_location + ": " + stocs_last_error());
    ModelCloud sampled;
    int n = 0;
    int rc = stocs_preprocess_model_mesh(mesh_v.data(), nv, mesh_t.data(), nt, spacing, seed, orient, voxel_size, read_depth_scale, -1, NULL, NULL, 0, &n);   // the size
    if (rc == STOCS_ERR_CAPACITY && n > 0) {
        sampled.pos.resize((size_t)n * 3); sampled.nrm.resize((size_t)n * 3);
        rc = stocs_preprocess_model_mesh(mesh_v.data(), nv, mesh_t.data(), nt, spacing, seed, orient, voxel_size, read_depth_scale, -1, sampled.pos.data(), sampled.nrm.data(), n, &n);
    }
    if (rc != STOCS_OK) throw std::runtime_error(std::string("stocs_preprocess_model_mesh: ") + stocs_last_error());
    write_model_and_index(sampled, n, write_depth_scale, ppf_tr_discretization, ppf_rot_discretization, dst_model_location, dst_ppf_map_location);
}

}  // namespace stocs

#endif
