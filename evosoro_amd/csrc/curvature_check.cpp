// Host-only check of the corner table k_shape_curvature walks (batch.hpp curvature_corner_table, device_types.hpp): no HIP, built with the
// plain C++ compiler (make curvature_check), so it also runs under the host sanitizers.  Exit status 0 = all consistent.
//   curvature_check <golden dir>     lw_swim6, lw_land6, lw_stiff5 of <golden dir>/vxa and a full 14^3 cube built on lw_swim6's settings
// Per robot: no group straddles a chunk, every facet corner of mesh_angle_excess's walk is in the table exactly once and nothing else is,
// and the angle excess evaluated THROUGH the table the way the kernel does -- one angle per record, a vertex's angles added left to right
// from 0.0 -- is mesh_angle_excess's bit for bit, in the rest state and in a deformed one.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "batch.hpp"
#include "engine.hpp"
#include "import.hpp"

using namespace vxh;

namespace {

const char* g_case = "";
[[noreturn]] void fail(const char* fmt, ...)
{
    std::fprintf(stderr, "curvature_check [%s]: ", g_case);
    va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
    std::fprintf(stderr, "\n");
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

struct Rec { int at, p, q, len, mark; };
Rec unpack(unsigned long long w) { return {(int)(w & 0xFFFF), (int)(w >> 16 & 0xFFFF), (int)(w >> 32 & 0xFFFF), (int)(w >> 48 & 0xFF), (int)(w >> 56)}; }

// the layout: groups whole inside a chunk, vertices ascending, every corner of the host's walk exactly once; returns the corners per vertex
std::vector<int> check_layout(const RobotModel& M, const std::vector<unsigned long long>& rec, int n_chunk)
{
    CHECK(n_chunk > 0 && rec.size() == (size_t)n_chunk * VXH_CURV_CHUNK, "%d chunks, %zu records", n_chunk, rec.size());
    std::map<std::tuple<int, int, int>, int> want;         // (at, p, q) -> how often the host's walk meets it
    std::vector<std::vector<std::pair<int, int>>> in_order((size_t)M.nmv);
    auto emit = [&](int at, int p, int q) { ++want[{at, p, q}]; in_order[at].push_back({p, q}); };
    for (size_t f = 0; f < M.facet_vert.size() / 3; ++f) {
        const int a = M.facet_vert[3 * f], b = M.facet_vert[3 * f + 1], c = M.facet_vert[3 * f + 2];
        emit(a, b, c);
        if (b != a) emit(b, a, c);
        if (c != a && c != b) emit(c, a, b);
    }
    std::vector<int> corners((size_t)M.nmv, 0);
    int next_vertex = 0;
    for (size_t k = 0; k < rec.size();) {
        const Rec h = unpack(rec[k]);
        if (h.mark == VXH_CURV_IDLE) { CHECK(h.len == 0, "record %zu: padding with a group length", k); ++k; continue; }
        CHECK(h.mark == 0 && h.len > 0 && h.at == next_vertex, "record %zu: expected the first corner of vertex %d, found at %d len %d mark %d", k, next_vertex, h.at, h.len, h.mark);
        CHECK(k / VXH_CURV_CHUNK == (k + h.len - 1) / VXH_CURV_CHUNK, "the group of vertex %d (records %zu..%zu) straddles a chunk", h.at, k, k + h.len - 1);
        CHECK((size_t)h.len == in_order[h.at].size(), "vertex %d: %d corners in the table, %zu in the walk", h.at, h.len, in_order[h.at].size());
        for (int j = 0; j < h.len; ++j) {
            const Rec r = unpack(rec[k + j]);
            CHECK(r.mark == 0 && r.at == h.at && (j == 0 || r.len == 0), "record %zu: not a corner of vertex %d", k + j, h.at);
            CHECK(r.p == in_order[h.at][j].first && r.q == in_order[h.at][j].second, "vertex %d corner %d: not in facet order", h.at, j);
            CHECK(--want[std::make_tuple(r.at, r.p, r.q)] >= 0, "corner (%d, %d, %d) more often than in the walk", r.at, r.p, r.q);
        }
        corners[h.at] = h.len;
        k += h.len; ++next_vertex;
    }
    CHECK(next_vertex == M.nmv, "%d of %d vertices have a group", next_vertex, M.nmv);
    for (const auto& w : want) CHECK(w.second == 0, "corner (%d, %d, %d) is missing", std::get<0>(w.first), std::get<1>(w.first), std::get<2>(w.first));
    return corners;
}

// as the kernel: one angle per record (angle_at of mesh_angle_excess), then the head of each group adds its angles left to right from 0.0
std::vector<double> through_the_table(const std::vector<double>& vert, const std::vector<unsigned long long>& rec, int nmv)
{
    std::vector<double> angle(rec.size(), 0.0), out((size_t)nmv, 0.0);
    for (size_t k = 0; k < rec.size(); ++k) {
        const Rec r = unpack(rec[k]);
        if (r.mark == VXH_CURV_IDLE) continue;
        double v1[3], v2[3];
        for (int c = 0; c < 3; ++c) { v1[c] = vert[(size_t)3 * r.p + c] - vert[(size_t)3 * r.at + c]; v2[c] = vert[(size_t)3 * r.q + c] - vert[(size_t)3 * r.at + c]; }
        const double l1 = std::sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]), l2 = std::sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
        if (l1 > 0) { v1[0] /= l1; v1[1] /= l1; v1[2] /= l1; }
        if (l2 > 0) { v2[0] /= l2; v2[1] /= l2; v2[2] /= l2; }
        angle[k] = std::acos(v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]);
    }
    for (size_t k = 0; k < rec.size(); ++k) {
        const Rec h = unpack(rec[k]);
        if (h.len == 0) continue;
        double sum = 0.0;
        for (int j = 0; j < h.len; ++j) sum = sum + angle[k + j];
        out[h.at] = (2.0 * 3.14159265358979) - sum;
    }
    return out;
}

void check_robot(const char* name, const RobotModel& M)
{
    g_case = name;
    std::vector<unsigned long long> rec(3, 0);             // (the function appends: a table behind another robot's)
    const int n_chunk = curvature_corner_table(M, rec);
    rec.erase(rec.begin(), rec.begin() + 3);
    const std::vector<int> corners = check_layout(M, rec, n_chunk);
    int most = 0;
    for (int c : corners) most = c > most ? c : most;
    // a deformed state: fixed pseudo-random displacements of a fifth of a voxel, rotations of up to ~0.3 rad, strains of up to 10 %
    unsigned long long seed = 0x9E3779B97F4A7C15ull;
    auto unit = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0 - 0.5; };
    std::vector<double> pos((size_t)3 * M.nvox), quat((size_t)4 * M.nvox), strain((size_t)6 * M.nvox);
    for (int v = 0; v < M.nvox; ++v) {
        for (int k = 0; k < 3; ++k) pos[(size_t)3 * v + k] = M.nom_pos[(size_t)3 * v + k] + 0.4 * unit() * M.vxa.lattice_dim;
        double q[4] = {1.0, 0.3 * unit(), 0.3 * unit(), 0.3 * unit()};
        const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int k = 0; k < 4; ++k) quat[(size_t)4 * v + k] = q[k] / l;
        for (int k = 0; k < 6; ++k) strain[(size_t)6 * v + k] = 0.2 * unit();
    }
    for (int deformed = 0; deformed < 2; ++deformed) {
        MeshShape sh;
        if (deformed) mesh_shape(M, pos.data(), quat.data(), strain.data(), sh); else mesh_shape(M, nullptr, nullptr, nullptr, sh);
        CHECK((int)sh.angle_excess.size() == M.nmv && (int)sh.verts.size() == 3 * M.nmv, "mesh_shape: %zu values for %d vertices", sh.angle_excess.size(), M.nmv);
        const std::vector<double> got = through_the_table(sh.verts, rec, M.nmv);
        for (int i = 0; i < M.nmv; ++i)
            CHECK(std::memcmp(&got[i], &sh.angle_excess[i], sizeof(double)) == 0, "%s state, vertex %d: %.17g through the table, %.17g from mesh_angle_excess",
                  deformed ? "deformed" : "rest", i, got[i], sh.angle_excess[i]);
    }
    std::printf("curvature_check %s: %d vertices, %zu corners in %d chunks (%zu padding), at most %d per vertex, rest and deformed state bit-equal: ok\n", name, M.nmv,
                M.facet_vert.size(), n_chunk, rec.size() - M.facet_vert.size(), most);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: curvature_check <golden dir>\n"); return 2; }
    const std::string golden = argv[1];
    const char* names[3] = {"lw_swim6", "lw_land6", "lw_stiff5"};
    std::vector<std::string> paths;
    for (const char* n : names) paths.push_back(golden + "/vxa/" + n + ".vxa");
    const std::vector<RobotModel> models = build_vxa_files(paths, 1, false);
    for (int k = 0; k < 3; ++k) check_robot(names[k], models[k]);
    // a full 14^3 cube, materials 3 / 4 in a checkerboard, on lw_swim6's settings: 1178 mesh vertices
    std::ifstream in(paths[0], std::ios::binary);
    std::stringstream text;
    text << in.rdbuf();
    const std::string tmpl = text.str();
    std::vector<unsigned char> material((size_t)14 * 14 * 14);
    for (int z = 0; z < 14; ++z) for (int y = 0; y < 14; ++y) for (int x = 0; x < 14; ++x) material[((size_t)z * 14 + y) * 14 + x] = (unsigned char)(3 + (x + y + z) % 2);
    vxh_robot_arrays A{};
    A.nx = A.ny = A.nz = 14; A.material = material.data();
    const std::vector<RobotModel> cube = build_arrays(tmpl.data(), tmpl.size(), &A, 1, false, 1, false);
    CHECK(cube.size() == 1 && cube[0].nmv == 1178, "the cube has %d mesh vertices", cube.empty() ? -1 : cube[0].nmv);
    check_robot("cube14", cube[0]);
    // what has no table
    g_case = "refusals";
    std::vector<unsigned long long> none;
    RobotModel big = cube[0];
    big.nmv = VXH_SHAPE_LARGE_MAX_VERT + 1;
    CHECK(curvature_corner_table(big, none) == 0 && none.empty(), "a mesh above the vertex cap has a table");
    RobotModel lonely = cube[0];
    lonely.nmv += 1;                                       // (a vertex no facet names)
    CHECK(curvature_corner_table(lonely, none) == 0 && none.empty(), "a vertex without corners has a table");
    std::printf("curvature_check: four robots, two refusals: ok\n");
    return 0;
}
