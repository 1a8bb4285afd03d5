// model_preprocess -- the repo's equivalent of the reference's offline tool (reference src/model_preprocess.cpp:14-39):
// models/<object>/textured_vertices.ply -> models/<object>/model_search.ply + models/<object>/ppf_map, through
// stocs::pre_process_model (normals, voxel grid and the O(|M|^2) PPF index all on the GPU).
//   model_preprocess <object_name> [--repo DIR] [--voxel 0.01] [--normal-radius 0.005] [--model-scale 1.0]
//                    [--find-symmetry [--sym-tol m] [--sym-steps n]]
//                    [--mesh <ply> [--spacing m] [--orient winding|origin] [--sample-seed n]]
// The reference edits these constants in the source per data set (README.md:42-60); the defaults are its YCB values.
// --find-symmetry (not in the reference): after the index is written, search the sampled model for its symmetry axes
// (stocs_find_symmetries; --sym-tol: the tolerance in metres, default a tenth of the diameter; --sym-steps: steps of a continuous axis,
// default 72), print them, write models/<object>/symmetry.txt -- the text stocs_single --sym-file reads: 16 floats per transform,
// column-major -- and print the --sym a,b,c line to use with it.
// --mesh <ply> (not in the reference): the model comes from a triangle mesh in place of textured_vertices.ply: its surface is sampled on
// the GPU at one point per spacing^2 (--spacing, in the mesh's units; default voxel / 4) with facet normals oriented by the winding
// (--orient origin: turned away from the origin, for meshes whose winding is not consistent), then voxel grid, scale and index as before;
// --normal-radius is not read.  A file that holds no mesh, or no faces, is refused.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../include/stocs.hpp"

static std::string repo_path = ".";
static float voxel_size = 0.01f;       // :7
static float normal_radius = 0.005f;   // :8
static float model_scale = 1.0f;       // :9
static int ppf_tr_discretization = 5;  // :12
static int ppf_rot_discretization = 5; // :13

int main(int argc, char** argv) {
    if (argc < 2) {
        std::cout << "Enter name of the object model!!" << std::endl;   // :18
        return -1;
    }
    const std::string object_name = argv[1];
    if (const char* e = getenv("STOCS_REPO_PATH")) repo_path = e;
    bool find_symmetry = false;
    stocs_symmetry_search search = stocs::default_symmetry_search();
    std::string mesh_path;
    float spacing = 0.0f;
    int orient = STOCS_MESH_ORIENT_WINDING;
    unsigned long long sample_seed = 0;
    bool have_mesh_option = false;
    for (int i = 2; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--find-symmetry") { find_symmetry = true; --i; continue; }   // a flag: no value
        if (i + 1 >= argc) break;   // a last option without its value is ignored, as it always was
        const std::string v = argv[i + 1];
        if (k == "--repo") repo_path = v;
        else if (k == "--sym-tol") search.tol_max = (float)atof(v.c_str());
        else if (k == "--sym-steps") search.n_continuous = atoi(v.c_str());
        else if (k == "--voxel") voxel_size = (float)atof(v.c_str());
        else if (k == "--normal-radius") normal_radius = (float)atof(v.c_str());
        else if (k == "--model-scale") model_scale = (float)atof(v.c_str());
        else if (k == "--mesh") mesh_path = v;
        else if (k == "--spacing") { spacing = (float)atof(v.c_str()); have_mesh_option = true; }
        else if (k == "--sample-seed") { sample_seed = strtoull(v.c_str(), NULL, 0); have_mesh_option = true; }
        else if (k == "--orient") {
            if (v != "winding" && v != "origin") { std::cerr << "--orient takes winding or origin" << std::endl; return -1; }
            orient = v == "origin" ? STOCS_MESH_ORIENT_ORIGIN : STOCS_MESH_ORIENT_WINDING;
            have_mesh_option = true;
        }
        else { std::cerr << "unknown option " << k << std::endl; return -1; }
    }
    if (have_mesh_option && mesh_path.empty()) { std::cerr << "--spacing, --orient and --sample-seed need --mesh <ply>" << std::endl; return -1; }
    const std::string model_path = repo_path + "/models/" + object_name;
    remove((model_path + "/model_search.ply").c_str());   // :25-26
    remove((model_path + "/ppf_map").c_str());
    try {
        if (!mesh_path.empty())
            stocs::pre_process_model_mesh(mesh_path, spacing, (uint64_t)sample_seed, orient, model_scale, 1.0f, voxel_size, ppf_tr_discretization, ppf_rot_discretization,
                                          model_path + "/model_search.ply", model_path + "/ppf_map");
        else
            stocs::pre_process_model(model_path + "/textured_vertices.ply", normal_radius, model_scale, 1.0f, voxel_size, ppf_tr_discretization, ppf_rot_discretization,
                                     model_path + "/model_search.ply", model_path + "/ppf_map");
        if (find_symmetry) {
            const stocs::SymmetryResult r = stocs::find_model_symmetries(model_path + "/model_search.ply", search);
            std::cout << "symmetry axes: " << r.axes.size() << std::endl;
            for (size_t k = 0; k < r.axes.size(); ++k) {
                const stocs_symmetry_axis& a = r.axes[k];
                char line[256];
                snprintf(line, sizeof line, "symmetry axis %zu: axis=%.6f,%.6f,%.6f order=%d max=%.6f mean=%.6f n_normal_bad=%d", k, (double)a.axis[0], (double)a.axis[1],
                         (double)a.axis[2], a.order, (double)a.max, (double)a.mean, a.n_normal_bad);
                std::cout << line << std::endl;
            }
            const std::string sym_path = model_path + "/symmetry.txt";
            std::ofstream f(sym_path.c_str());
            for (size_t k = 0; k < r.set16.size() / 16; ++k) {
                for (int e = 0; e < 16; ++e) {
                    char num[32];
                    snprintf(num, sizeof num, "%.9g", (double)r.set16[k * 16 + e]);
                    f << num << (e == 15 ? "\n" : " ");
                }
            }
            f.close();
            if (!f) { std::cerr << "cannot write " << sym_path << std::endl; return 2; }
            std::cout << "symmetry set: " << r.set16.size() / 16 << " transforms -> " << sym_path
                      << ((r.flags & STOCS_SYMMETRY_SET_TRUNCATED) ? " (truncated)" : "") << ((r.flags & STOCS_SYMMETRY_NOTHING_FOUND) ? " (nothing found: the identity)" : "") << std::endl;
            std::cout << "use: --sym " << r.sym3[0] << "," << r.sym3[1] << "," << r.sym3[2] << " --sym-file " << sym_path
                      << ((r.flags & STOCS_SYMMETRY_DESCRIPTOR_INEXACT) ? "   (the descriptor cannot name these axes: cluster without it, evaluate with the file)" : "") << std::endl;
        }
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;   // no GPU => loud failure
        return 2;
    }
    return 0;
}
