// Import pipeline (import.hpp).  Host-only code.
#include "import.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace vxh {

namespace {

// A generation arrives as hundreds of robots; reading, XML parsing and model building (hop-distance lists, bond classes, drag mesh) are
// independent per robot and take longer than the GPU needs to simulate them, so they are spread over the host cores.
// 32 workers: on the 256-thread MI355X host 512 robots import in 15 ms with 32 threads and in 200 ms with 64 (allocator contention)
constexpr int IMPORT_THREADS = 32;

// the per-voxel layers a robot handed over as arrays may carry
struct LayerSlot { const char* tag; bool VxaModel::*has; std::vector<double> VxaModel::*values; bool land_only; };
const LayerSlot layer_slots[] = {
    {"PhaseOffset", &VxaModel::has_phase_offset, &VxaModel::phase_offset, false}, {"TempAmpDamp", &VxaModel::has_temp_amp_damp, &VxaModel::temp_amp_damp, false},
    {"Stiffness", &VxaModel::has_stiffness, &VxaModel::stiffness, false}, {"FinalPhaseOffset", &VxaModel::has_final_phase_offset, &VxaModel::final_phase_offset, true},
    {"FinalTempAmpDamp", &VxaModel::has_final_temp_amp_damp, &VxaModel::final_temp_amp_damp, true}, {"InitialVoxelSize", &VxaModel::has_initial_voxel_size, &VxaModel::initial_voxel_size, true},
    {"FinalVoxelSize", &VxaModel::has_final_voxel_size, &VxaModel::final_voxel_size, true}, {"GrowthTime", &VxaModel::has_growth_time, &VxaModel::growth_time, true},
    {"StartGrowthTime", &VxaModel::has_start_growth_time, &VxaModel::start_growth_time, true},
};

// The VxaModel of a robot handed over as arrays is exactly what read_vxa builds from the file the writer would have produced: the
// template's settings (`base`), material digits as they are, layer values taken by occupied-voxel counter in file order
// (VX_Object.cpp:1879-1900), optionally through the writer's decimal text.
VxaModel model_from_arrays(const VxaModel& base, const vxh_robot_arrays& A, int variant, bool round_like_text)
{
    if (A.nx < 1 || A.ny < 1 || A.nz < 1 || (long long)A.nx * A.ny * A.nz > (1LL << 26) || !A.material) throw std::invalid_argument("bad lattice");
    if (A.n_layers < 0 || (A.n_layers > 0 && (!A.layer_tags || !A.layers))) throw std::invalid_argument("bad layer arrays");
    for (int l = 0; l < A.n_layers; ++l) if (!A.layer_tags[l] || !A.layers[l]) throw std::invalid_argument("null layer tag or layer");
    VxaModel m = base;
    m.nx = A.nx; m.ny = A.ny; m.nz = A.nz;
    const size_t cells = (size_t)A.nx * A.ny * A.nz;
    m.structure.assign(A.material, A.material + cells);
    for (size_t k = 0; k < cells; ++k)
        if (m.structure[k] >= m.palette.size()) throw std::invalid_argument("material index outside the palette");
    if (A.fitness_file_name) m.fitness_file_name = A.fitness_file_name;
    for (int l = 0; l < A.n_layers; ++l) {
        const LayerSlot* slot = nullptr;
        for (const auto& sl : layer_slots) if (std::strcmp(sl.tag, A.layer_tags[l]) == 0) slot = &sl;
        if (!slot) throw std::invalid_argument(std::string("unsupported per-voxel layer <") + A.layer_tags[l] + ">");
        if (slot->land_only && variant != 0) throw std::invalid_argument(std::string("unsupported <") + A.layer_tags[l] + "> development layer (land_water)");
        std::vector<double>& out = m.*(slot->values);
        m.*(slot->has) = true;
        out.clear();
        for (size_t k = 0; k < cells; ++k) {
            if (m.structure[k] == 0) continue;
            double v = A.layers[l][k];
            if (round_like_text) { char buf[48]; std::snprintf(buf, sizeof(buf), "%.12g", v); v = std::atof(buf); }
            out.push_back(v);
        }
    }
    return m;
}

}  // namespace

VxaModel read_supported_vxa(const char* data, size_t len, int variant, bool want_mesh, const std::string& where)
{
    VxaModel vxa = read_vxa(data, len, variant);
    if (want_mesh) vxa.want_mesh = true;
    if (!vxa.unsupported.empty()) {
        std::string msg = "unsupported .vxa feature(s):";
        for (const auto& u : vxa.unsupported) msg += " [" + u + "]";
        throw std::invalid_argument(msg + where);
    }
    return vxa;
}

std::vector<RobotModel> build_vxa(const char* data, size_t len, int variant, bool want_mesh)
{
    std::vector<RobotModel> out;
    out.push_back(build_robot(read_supported_vxa(data, len, variant, want_mesh, "")));
    return out;
}

std::vector<RobotModel> build_vxa_files(const std::vector<std::string>& paths, int variant, bool want_mesh)
{
    std::vector<RobotModel> built(paths.size());
    for_each_index((int)paths.size(), IMPORT_THREADS, [&](int i) {
        std::ifstream in(paths[i], std::ios::binary);
        if (!in) throw std::runtime_error("io: cannot open " + paths[i]);
        std::stringstream ss;
        ss << in.rdbuf();
        const std::string text = ss.str();
        built[i] = build_robot(read_supported_vxa(text.data(), text.size(), variant, want_mesh, " in " + paths[i]));
    });
    return built;
}

std::vector<VxaModel> models_from_arrays(const char* template_vxa, size_t len, const vxh_robot_arrays* in, int n, bool round_like_text, int variant, bool want_mesh)
{
    VxaModel base = read_supported_vxa(template_vxa, len, variant, want_mesh, " in the template");
    for (const auto& sl : layer_slots) { base.*(sl.has) = false; (base.*(sl.values)).clear(); }
    base.structure.clear();
    std::vector<VxaModel> built(std::max(n, 0));
    for_each_index(n, IMPORT_THREADS, [&](int i) { built[i] = model_from_arrays(base, in[i], variant, round_like_text); });
    return built;
}

std::vector<RobotModel> build_models(std::vector<VxaModel>&& models)
{
    std::vector<RobotModel> built(models.size());
    for_each_index((int)models.size(), IMPORT_THREADS, [&](int i) { built[i] = build_robot(models[i]); });
    return built;
}

std::vector<RobotModel> build_arrays(const char* template_vxa, size_t len, const vxh_robot_arrays* in, int n, bool round_like_text, int variant, bool want_mesh)
{
    return build_models(models_from_arrays(template_vxa, len, in, n, round_like_text, variant, want_mesh));
}

}  // namespace vxh
