// Fitness metrics and result XML.  Reference: CVX_SimGA::WriteResultFile (evosoro/_voxcad/Voxelyze/VX_SimGA.cpp:33-203;
// land_water: evosoro/_voxcad_land_water/Voxelyze/VX_SimGA.cpp:33-77), the SS.* values of CVX_Sim::UpdateStats
// (VX_Sim.cpp:1518-1535) with their helpers GetCM / getAnteriorDist / getPosteriorY / GetNumTouchingFloor
// (VX_Sim.cpp:2415-2441,2584-2712).  Numbers are printed like `ostream << double` (6 significant digits,
// Utils/XML_Rip.h:57) in TinyXML's layout (4 blanks per level).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>
#include <cstdio>
#include <cstring>

#include "engine.hpp"

namespace vxh {

namespace {

// CVX_MeshUtil::computeCurrentRobotVolume (LW/VX_MeshUtil.cpp:908-952): signed tetrahedra over the facets of the
// deformable surface mesh; vertices as updateDeformableMesh / GetCurVLoc (:368-428) places them: mean over the voxels
// touching the lattice corner of Pos + R(Angle) * corner, corner = +-(1 + strain) * L / 2.  `pos` etc. may be null:
// the rest state (RobotVolumeStart is taken right after Import, voxelyzeMain/main.cpp:65).
double robot_volume(const RobotModel& M, const double* pos, const double* quat, const double* strain)
{
    if (M.nmv == 0) return 0.0;
    const double nom = M.vxa.lattice_dim;
    std::vector<double> vert((size_t)M.nmv * 3);
    for (int i = 0; i < M.nmv; ++i) {
        double ax = 0, ay = 0, az = 0, tw = 0;
        for (int q = 0; q < 8; ++q) {
            const int comp = M.vert_comp[(size_t)i * 8 + q];
            if (comp < 0) break;
            const int u = comp >> 3, corner = comp & 7;
            double st[6] = {0, 0, 0, 0, 0, 0};
            if (strain) for (int k = 0; k < 6; ++k) st[k] = strain[(size_t)6 * u + k];
            const double ox = (corner & 4) ? (1 + st[0]) * nom * 0.5 : -(1 + st[3]) * nom * 0.5;
            const double oy = (corner & 2) ? (1 + st[1]) * nom * 0.5 : -(1 + st[4]) * nom * 0.5;
            const double oz = (corner & 1) ? (1 + st[2]) * nom * 0.5 : -(1 + st[5]) * nom * 0.5;
            double px = M.nom_pos[3 * u], py = M.nom_pos[3 * u + 1], pz = M.nom_pos[3 * u + 2];
            double qw = 1, qx = 0, qy = 0, qz = 0;
            if (pos) { px = pos[3 * u]; py = pos[3 * u + 1]; pz = pos[3 * u + 2]; qw = quat[4 * u]; qx = quat[4 * u + 1]; qy = quat[4 * u + 2]; qz = quat[4 * u + 3]; }
            // CQuat::RotateVec3D, Vec3D.h:293-299
            const double tw_ = ox * qx + oy * qy + oz * qz, tx = ox * qw - oy * qz + oz * qy, ty = ox * qz + oy * qw - oz * qx, tz = -ox * qy + oy * qx + oz * qw;
            ax += px + (qw * tx + qx * tw_ + qy * tz - qz * ty);
            ay += py + (qw * ty - qx * tz + qy * tw_ + qz * tx);
            az += pz + (qw * tz + qx * ty - qy * tx + qz * tw_);
            tw += 1.0;
        }
        const double inv = 1.0 / tw;
        const double v0x = M.vert_v0[(size_t)3 * i], v0y = M.vert_v0[(size_t)3 * i + 1], v0z = M.vert_v0[(size_t)3 * i + 2];
        vert[(size_t)3 * i] = v0x + (ax * inv - v0x); vert[(size_t)3 * i + 1] = v0y + (ay * inv - v0y); vert[(size_t)3 * i + 2] = v0z + (az * inv - v0z);
    }
    // corner codes (NNN..PPP) of the two triangles of faces +X,-X,+Y,-Y,+Z,-Z (LW/VX_MeshUtil.cpp:165-189)
    static const unsigned tri[6][2] = {{0x467u, 0x475u}, {0x032u, 0x013u}, {0x237u, 0x276u}, {0x051u, 0x045u}, {0x157u, 0x173u}, {0x064u, 0x026u}};
    double volume = 0.0;
    for (int v = 0; v < M.nvox; ++v)
        for (int d = 0; d < 6; ++d) {
            if (!(M.open_face[v] & (1u << d))) continue;
            for (int t = 0; t < 2; ++t) {
                const unsigned code = tri[d][t];
                const double* a = &vert[(size_t)3 * M.corner_vert[(size_t)v * 8 + ((code >> 8) & 7u)]];
                const double* b = &vert[(size_t)3 * M.corner_vert[(size_t)v * 8 + ((code >> 4) & 7u)]];
                const double* c = &vert[(size_t)3 * M.corner_vert[(size_t)v * 8 + (code & 7u)]];
                const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
                volume += (1.0 / 6.0) * (cx * c[0] + cy * c[1] + cz * c[2]);
            }
        }
    return volume;
}

// vertices of the deformable surface mesh (rest state when pos == null), as robot_volume places them
void mesh_vertices(const RobotModel& M, const double* pos, const double* quat, const double* strain, std::vector<double>& vert)
{
    const double nom = M.vxa.lattice_dim;
    vert.assign((size_t)M.nmv * 3, 0.0);
    for (int i = 0; i < M.nmv; ++i) {
        double ax = 0, ay = 0, az = 0, tw = 0;
        for (int q = 0; q < 8; ++q) {
            const int comp = M.vert_comp[(size_t)i * 8 + q];
            if (comp < 0) break;
            const int u = comp >> 3, corner = comp & 7;
            double st[6] = {0, 0, 0, 0, 0, 0};
            if (strain) for (int k = 0; k < 6; ++k) st[k] = strain[(size_t)6 * u + k];
            const double ox = (corner & 4) ? (1 + st[0]) * nom * 0.5 : -(1 + st[3]) * nom * 0.5;
            const double oy = (corner & 2) ? (1 + st[1]) * nom * 0.5 : -(1 + st[4]) * nom * 0.5;
            const double oz = (corner & 1) ? (1 + st[2]) * nom * 0.5 : -(1 + st[5]) * nom * 0.5;
            double px = M.nom_pos[3 * u], py = M.nom_pos[3 * u + 1], pz = M.nom_pos[3 * u + 2];
            double qw = 1, qx = 0, qy = 0, qz = 0;
            if (pos) { px = pos[3 * u]; py = pos[3 * u + 1]; pz = pos[3 * u + 2]; qw = quat[4 * u]; qx = quat[4 * u + 1]; qy = quat[4 * u + 2]; qz = quat[4 * u + 3]; }
            const double tw_ = ox * qx + oy * qy + oz * qz, tx = ox * qw - oy * qz + oz * qy, ty = ox * qz + oy * qw - oz * qx, tz = -ox * qy + oy * qx + oz * qw;
            ax += px + (qw * tx + qx * tw_ + qy * tz - qz * ty);
            ay += py + (qw * ty - qx * tz + qy * tw_ + qz * tx);
            az += pz + (qw * tz + qx * ty - qy * tx + qz * tw_);
            tw += 1.0;
        }
        const double inv = 1.0 / tw;
        const double v0x = M.vert_v0[(size_t)3 * i], v0y = M.vert_v0[(size_t)3 * i + 1], v0z = M.vert_v0[(size_t)3 * i + 2];
        vert[(size_t)3 * i] = v0x + (ax * inv - v0x); vert[(size_t)3 * i + 1] = v0y + (ay * inv - v0y); vert[(size_t)3 * i + 2] = v0z + (az * inv - v0z);
    }
}

}  // namespace

// Volume of the convex hull of a point set: what the reference obtains by writing the mesh vertices to a file and running the external
// `qhull FS` on it (CVX_MeshUtil::writeQhullInputFile / invokeQhull, LW/VX_MeshUtil.cpp:775-900).  Incremental hull: a tetrahedron of
// four points in general position, then every point that lies outside replaces the faces it sees by a cone over their horizon.  A
// point closer to a face plane than `eps` counts as not seeing it: lattice corners make thousands of coplanar points, and the volume
// does not notice the difference.  O(points x faces), a few hundred of each here.
double convex_hull_volume(const std::vector<double>& pts)
{
    const int n = (int)(pts.size() / 3);
    if (n < 4) return 0.0;
    auto P = [&](int i) { return &pts[(size_t)3 * i]; };
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], P(i)[k]); hi[k] = std::max(hi[k], P(i)[k]); }
    const double diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    if (!(diag > 0)) return 0.0;
    const double eps = 1e-9 * diag;
    struct Face { int a, b, c; double nx, ny, nz, d; bool alive; };
    auto make = [&](int a, int b, int c) {
        const double *A = P(a), *B = P(b), *C = P(c);
        const double ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2], vx = C[0] - A[0], vy = C[1] - A[1], vz = C[2] - A[2];
        double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double l = std::sqrt(nx * nx + ny * ny + nz * nz);
        if (l > 0) { nx /= l; ny /= l; nz /= l; }
        return Face{a, b, c, nx, ny, nz, nx * A[0] + ny * A[1] + nz * A[2], true};
    };
    auto dist = [&](const Face& f, int i) { return f.nx * P(i)[0] + f.ny * P(i)[1] + f.nz * P(i)[2] - f.d; };
    // initial tetrahedron: extreme points along x, the point farthest from that line, the point farthest from that plane
    int i0 = 0, i1 = 0;
    for (int i = 0; i < n; ++i) { if (P(i)[0] < P(i0)[0]) i0 = i; if (P(i)[0] > P(i1)[0]) i1 = i; }
    if (i0 == i1) { for (int i = 0; i < n; ++i) { if (P(i)[1] < P(i0)[1]) i0 = i; if (P(i)[1] > P(i1)[1]) i1 = i; } }
    if (i0 == i1) { for (int i = 0; i < n; ++i) { if (P(i)[2] < P(i0)[2]) i0 = i; if (P(i)[2] > P(i1)[2]) i1 = i; } }
    if (i0 == i1) return 0.0;
    int i2 = -1; double best = 0;
    {
        const double ex = P(i1)[0] - P(i0)[0], ey = P(i1)[1] - P(i0)[1], ez = P(i1)[2] - P(i0)[2];
        for (int i = 0; i < n; ++i) {
            const double px = P(i)[0] - P(i0)[0], py = P(i)[1] - P(i0)[1], pz = P(i)[2] - P(i0)[2];
            const double cx = ey * pz - ez * py, cy = ez * px - ex * pz, cz = ex * py - ey * px, a2 = cx * cx + cy * cy + cz * cz;
            if (a2 > best) { best = a2; i2 = i; }
        }
    }
    if (i2 < 0 || !(std::sqrt(best) > eps * diag)) return 0.0;
    Face base = make(i0, i1, i2);
    int i3 = -1; best = 0;
    for (int i = 0; i < n; ++i) { const double h = std::fabs(dist(base, i)); if (h > best) { best = h; i3 = i; } }
    if (i3 < 0 || !(best > eps)) return 0.0;                          // all points in one plane
    std::vector<Face> faces;
    if (dist(base, i3) > 0) std::swap(i1, i2);                        // orient (i0, i1, i2) away from i3
    faces.push_back(make(i0, i1, i2)); faces.push_back(make(i0, i3, i1)); faces.push_back(make(i1, i3, i2)); faces.push_back(make(i2, i3, i0));
    std::vector<char> sees;
    std::vector<std::pair<int, int>> horizon;
    for (int p = 0; p < n; ++p) {
        if (p == i0 || p == i1 || p == i2 || p == i3) continue;
        sees.assign(faces.size(), 0);
        bool any = false;
        for (size_t f = 0; f < faces.size(); ++f) if (faces[f].alive && dist(faces[f], p) > eps) { sees[f] = 1; any = true; }
        if (!any) continue;
        // horizon: the directed edges of visible faces whose twin belongs to a face that is not visible
        horizon.clear();
        for (size_t f = 0; f < faces.size(); ++f) {
            if (!sees[f]) continue;
            const int e[3][2] = {{faces[f].a, faces[f].b}, {faces[f].b, faces[f].c}, {faces[f].c, faces[f].a}};
            for (int k = 0; k < 3; ++k) {
                bool twin_visible = false;
                for (size_t g = 0; g < faces.size() && !twin_visible; ++g) {
                    if (!sees[g] || g == f) continue;
                    const Face& G = faces[g];
                    twin_visible = (G.a == e[k][1] && G.b == e[k][0]) || (G.b == e[k][1] && G.c == e[k][0]) || (G.c == e[k][1] && G.a == e[k][0]);
                }
                if (!twin_visible) horizon.push_back({e[k][0], e[k][1]});
            }
        }
        for (size_t f = 0; f < faces.size(); ++f) if (sees[f]) faces[f].alive = false;
        for (const auto& e : horizon) faces.push_back(make(e.first, e.second, p));
        if (faces.size() > 4096) {                                    // compact now and then
            std::vector<Face> live;
            for (const Face& f : faces) if (f.alive) live.push_back(f);
            faces.swap(live);
        }
    }
    // signed tetrahedra against an interior point
    const double cx = 0.25 * (P(i0)[0] + P(i1)[0] + P(i2)[0] + P(i3)[0]), cy = 0.25 * (P(i0)[1] + P(i1)[1] + P(i2)[1] + P(i3)[1]),
                 cz = 0.25 * (P(i0)[2] + P(i1)[2] + P(i2)[2] + P(i3)[2]);
    double volume = 0;
    for (const Face& f : faces) {
        if (!f.alive) continue;
        const double a[3] = {P(f.a)[0] - cx, P(f.a)[1] - cy, P(f.a)[2] - cz}, b[3] = {P(f.b)[0] - cx, P(f.b)[1] - cy, P(f.b)[2] - cz},
                     c[3] = {P(f.c)[0] - cx, P(f.c)[1] - cy, P(f.c)[2] - cz};
        volume += (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0])) / 6.0;
    }
    return std::fabs(volume);
}

// Angle excess 2 pi - (sum of the facet angles meeting in the vertex) of every vertex of the deformable surface mesh: the discrete
// curvatures CVX_MeshUtil::computeShapeComplexity (LW/VX_MeshUtil.cpp:956-1014) writes to <CurvaturesTmpFile> for the entropy script
// (which the reference repository does not contain).  Same operation order: a vertex adds the angles of its facets in facet order
// (the reference loops vertex-major and scans all facets per vertex -- O(V F); here one pass over the facets adds each facet's three
// angles to its three vertices, which visits a vertex's facets in the same order); edge vectors normalised with Vec3D::Normalize
// (sqrt, three divisions), angle = acos of their dot product, PI = 3.14159265358979 (Vec3D.h).
void mesh_angle_excess(const RobotModel& M, const double* pos, const double* quat, const double* strain, std::vector<double>& out)
{
    out.assign((size_t)M.nmv, 0.0);
    if (M.nmv == 0) return;
    std::vector<double> vert;
    mesh_vertices(M, pos, quat, strain, vert);
    std::vector<double> sum((size_t)M.nmv, 0.0);
    const size_t nf = M.facet_vox.size();
    auto angle_at = [&](int at, int p, int q) {
        double v1[3], v2[3];
        for (int k = 0; k < 3; ++k) { v1[k] = vert[(size_t)3 * p + k] - vert[(size_t)3 * at + k]; v2[k] = vert[(size_t)3 * q + k] - vert[(size_t)3 * at + k]; }
        const double l1 = std::sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]), l2 = std::sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
        if (l1 > 0) { v1[0] /= l1; v1[1] /= l1; v1[2] /= l1; }
        if (l2 > 0) { v2[0] /= l2; v2[1] /= l2; v2[2] /= l2; }
        return std::acos(v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]);
    };
    for (size_t f = 0; f < nf; ++f) {
        const int a = M.facet_vert[3 * f], b = M.facet_vert[3 * f + 1], c = M.facet_vert[3 * f + 2];
        // (`if V == a ... else if V == b ... else if V == c`: a vertex listed twice by a facet is counted once, as its first role)
        sum[a] += angle_at(a, b, c);
        if (b != a) sum[b] += angle_at(b, a, c);
        if (c != a && c != b) sum[c] += angle_at(c, a, b);
    }
    for (int i = 0; i < M.nmv; ++i) out[i] = (2.0 * 3.14159265358979) - sum[i];
}

// <ConvexHullVolumeStart/End> of a land_water robot: the hull of its surface-mesh vertices as the reference hands them to qhull,
// i.e. printed with the stream's 6 significant digits (LW/VX_MeshUtil.cpp:806)
double robot_hull_volume(const RobotModel& M, const double* pos, const double* quat, const double* strain)
{
    if (M.nmv == 0) return 0.0;
    std::vector<double> vert;
    mesh_vertices(M, pos, quat, strain, vert);
    for (double& v : vert) { char buf[48]; std::snprintf(buf, sizeof(buf), "%g", v); v = std::atof(buf); }
    return convex_hull_volume(vert);
}

void mesh_shape(const RobotModel& M, const double* pos, const double* quat, const double* strain, MeshShape& out)
{
    out = MeshShape();
    if (M.nmv == 0) return;
    mesh_vertices(M, pos, quat, strain, out.verts);
    out.facets.assign(M.facet_vert.begin(), M.facet_vert.end());
    out.robot_volume = robot_volume(M, pos, quat, strain);
    out.hull_volume = robot_hull_volume(M, pos, quat, strain);
    mesh_angle_excess(M, pos, quat, strain, out.angle_excess);
}

void compute_result(const RobotModel& M, const HostState& S, vxh_result* r)
{
    std::memset(r, 0, sizeof(*r));
    const VxaModel& X = M.vxa;
    r->status = S.status; r->steps = S.steps; r->nvox = M.nvox; r->nbond = M.nbond;
    r->dt = M.dt; r->cur_time = S.cur_time; r->col_rebuilds = S.rebuilds;
    const double lat = X.lattice_dim;
    // SS.CurCM after the last UpdateStats: sequential mass-weighted sum in voxel order (GetCM); zero before any step
    double cm[3] = {0, 0, 0};
    if (S.reduced) {                         // (k_results: the same sums, formed on the device in the same order)
        if (S.steps > 0 && M.nvox > 0) for (int k = 0; k < 3; ++k) cm[k] = S.red_cm[k];
    } else if (S.steps > 0 && M.nvox > 0) {
        double sx = 0, sy = 0, sz = 0, tm = 0;
        for (int v = 0; v < M.nvox; ++v) {
            const double m = M.vox_classes[M.vox_class[v]].mass;
            sx += S.pos[3 * v] * m; sy += S.pos[3 * v + 1] * m; sz += S.pos[3 * v + 2] * m; tm += m;
        }
        const double inv = 1.0 / tm;
        cm[0] = inv * sx; cm[1] = inv * sy; cm[2] = inv * sz;
    }
    for (int k = 0; k < 3; ++k) { r->cur_cm[k] = cm[k]; r->ini_cm[k] = S.ini_cm[k]; }
    if (X.variant == 0) {
        r->lifetime = S.cur_time - X.afterlife_time;
        const double fd = std::pow(std::pow(cm[0] - S.ini_cm[0], 2) + std::pow(cm[1] - S.ini_cm[1], 2), 0.5) / lat;
        double ant = 0.0, post = 100000.0, anty = 0.0, posty = 100000.0;
        int touching = 0, feet = 0;
        if (S.reduced) {
            // the extrema were taken on the device over the arguments; pow(., 0.5), the division by the lattice constant and the
            // comparisons with the start values (0 and 100000) are monotone, so they commute with max / min
            if (M.nvox > 0) {
                const double a = std::pow(S.d2max, 0.5) / lat, p = std::pow(S.d2min, 0.5) / lat;
                if (a > ant) ant = a;
                if (p < post) post = p;
                if (S.ymax > -1.0e299) { const double y1 = S.ymax / lat, y0 = S.ymin / lat; if (y1 > anty) anty = y1; if (y0 < posty) posty = y0; }
            }
            touching = S.touching; feet = S.feet;
        }
        for (int v = 0; v < (S.reduced ? 0 : M.nvox); ++v) {
            const VoxClass& C = M.vox_classes[M.vox_class[v]];
            const double x = S.pos[3 * v], y = S.pos[3 * v + 1], z = S.pos[3 * v + 2];
            const double d = std::pow(std::pow(x - S.ini_cm[0], 2) + std::pow(y - S.ini_cm[1], 2), 0.5) / lat;
            if (d > ant) ant = d;
            if (d < post) post = d;
            if (C.mat != 5) { const double yy = y / lat; if (yy > anty) anty = yy; if (yy < posty) posty = yy; }
            const double pen = 0.5 * S.scale[v] - z;
            if (pen > 0) { ++touching; if (C.mat == 6) ++feet; }
        }
        if (S.steps == 0) { ant = post = anty = posty = 0; touching = feet = 0; }   // SimState::Clear()
        r->final_dist = fd; r->norm_final_dist = fd; r->norm_frozen_dist = 0;
        r->norm_regime_dist = post - S.eol_post_y;
        if (X.norm_dist_by_vol) {
            // VX_SimGA.cpp:57-112: distance per trace interval over the robot's volume in it, from the traces the device recorded.  Where the
            // reference would read element [0] of an EMPTY trace (undefined behaviour) the sum is 0.
            const double e = X.normalization_exponent;
            const size_t n = std::min(S.cm_trace.size() / 4, S.vol_trace.size());
            r->norm_final_dist = norm_dist_by_vol(n, S.cm_trace.data() + 2, 4, S.vol_trace.data(), 1, lat, e);
            if (X.afterlife_time > 0) r->norm_regime_dist = norm_dist_by_vol(S.xtrace[0].size() / 5, S.xtrace[0].data() + 2, 5, S.xtrace[0].data() + 4, 5, lat, e);
            if (X.midlife_freeze_time > 0) r->norm_frozen_dist = norm_dist_by_vol(S.xtrace[1].size() / 5, S.xtrace[1].data() + 2, 5, S.xtrace[1].data() + 4, 5, lat, e);
        }
        r->final_dist_y = (cm[1] - S.ini_cm[1]) / lat;
        r->anterior_dist = ant; r->posterior_dist = post; r->anterior_y = anty; r->posterior_y = posty;
        r->end_of_life_posterior_y = S.eol_post_y; r->fall_adj_post_y = S.eol_post_y;
        r->num_non_feet_touching_floor = feet; r->num_touching_floor = touching;
    } else {
        r->lifetime = S.cur_time;
        const double inv = 1.0 / lat;
        const double dx = inv * (cm[0] - S.ini_cm[0]), dy = inv * (cm[1] - S.ini_cm[1]), dz = inv * (cm[2] - S.ini_cm[2]);
        r->norm_dist_x = (float)dx; r->norm_dist_y = (float)dy; r->norm_dist_z = (float)dz;   // float-typed in the reference
        r->norm_abs_disp = (float)std::sqrt(dx * dx + dy * dy + dz * dz);
        r->robot_volume_start = robot_volume(M, nullptr, nullptr, nullptr);
        r->hull_volume_start = robot_hull_volume(M, nullptr, nullptr, nullptr);
        const bool have = (int)S.strain.size() == 6 * M.nvox;
        if (S.steps == 0) { r->robot_volume_end = r->robot_volume_start; r->hull_volume_end = r->hull_volume_start; }
        else {
            r->robot_volume_end = have ? robot_volume(M, S.pos.data(), S.quat.data(), S.strain.data()) : -1.0;
            r->hull_volume_end = have ? robot_hull_volume(M, S.pos.data(), S.quat.data(), S.strain.data()) : -1.0;
        }
    }
}

namespace {
void tag(std::string& out, const char* name, double value)
{
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%g", value);
    out += "        <"; out += name; out += ">"; out += buf; out += "</"; out += name; out += ">\n";
}
}  // namespace

const std::vector<double>& empty_trace() { static const std::vector<double> none; return none; }

// the loop of VX_SimGA.cpp:59-73 (and :78-92, :97-111), operation for operation
double norm_dist_by_vol(size_t n, const double* y, size_t y_stride, const double* vol, size_t vol_stride, double lattice_dim, double exponent)
{
    if (n < 2) return 0.0;
    double last_y = y[0], last_vol = vol[0], sum = 0;
    for (size_t i = 1; i != n; ++i) {
        const double this_dist = (y[i * y_stride] - last_y) / lattice_dim;
        const double this_vol = (vol[i * vol_stride] + last_vol) / 2;
        sum += this_dist / std::pow(this_vol, exponent);
        last_y = y[i * y_stride]; last_vol = vol[i * vol_stride];
    }
    return sum;
}

// <ShapeComplexityStart/End> as the reference binary prints them when it is built from its repository: computeShapeComplexity
// (LW/VX_MeshUtil.cpp:1016-1076) writes the angle excesses to <CurvaturesTmpFile> (six significant digits each, tab-separated), runs
// `python <base>/../curvatureEntropy.py <file>` -- a script the repository does not contain, so the call fails and the file stays as it
// is --, waits a second and reads ONE number back from the file: the first vertex's angle excess as printed.  (Seen in every result
// file the reference writes here: tests/golden/expected/lw_*.xml carry the first value of their *.curv_start / *.curv_end vectors.)
// -1 where the reference returns it: no <CurvaturesTmpFile>, no vertex, a value the stream extraction rejects.
double shape_complexity_as_the_reference_prints_it(const RobotModel& M, const std::vector<double>& angle_excess)
{
    if (M.vxa.curvatures_tmp_file.empty() || angle_excess.empty()) return -1.0;
    char text[64];
    std::snprintf(text, sizeof(text), "%g", angle_excess[0]);
    if (!std::isfinite(angle_excess[0])) return -1.0;            // ("nan" / "inf": operator>> fails and leaves the -1 it started from)
    return std::strtod(text, nullptr);
}

std::string result_xml(const RobotModel& M, const vxh_result& r, const std::vector<double>& cm_trace, double shape_start, double shape_end,
                       const std::vector<double>& vol_trace)
{
    std::string out = "<?xml version=\"1.0\" ?>\n<Voxelyze_Sim_Result Version=\"1.0\">\n    <Fitness>\n";
    if (M.vxa.variant == 0) {
        tag(out, "NormFinalDist", r.norm_final_dist - r.norm_frozen_dist);
        tag(out, "NormRegimeDist", r.norm_regime_dist);
        tag(out, "NormFrozenDist", r.norm_frozen_dist);
        tag(out, "FinalDist", r.final_dist);
        tag(out, "finalDistY", r.final_dist_y);
        tag(out, "AnteriorDist", r.anterior_dist);
        tag(out, "PosteriorDist", r.posterior_dist);
        tag(out, "AnteriorY", r.anterior_y);
        tag(out, "PosteriorY", r.posterior_y);
        tag(out, "EndOfLifePosteriorY", r.end_of_life_posterior_y);
        tag(out, "FallAdjPostY", r.fall_adj_post_y);
        tag(out, "NumNonFeetTouchingFloor", r.num_non_feet_touching_floor);
        tag(out, "NumTouchingFloor", r.num_touching_floor);
        tag(out, "Lifetime", r.lifetime);
        tag(out, "FoundNeedleInHaystack", 0);
        tag(out, "PushDist", 0);
    } else {
        tag(out, "VoxelNumber", r.nvox);
        tag(out, "normAbsoluteDisplacement", r.norm_abs_disp);
        tag(out, "normDistX", r.norm_dist_x);
        tag(out, "normDistY", r.norm_dist_y);
        tag(out, "normDistZ", r.norm_dist_z);
        // the hull volumes: the reference shells out to qhull (and prints -1 when that is not installed), here computed in place;
        // the shape complexity: what the reference prints without its absent entropy script (shape_complexity_as_the_reference_prints_it)
        tag(out, "RobotVolumeStart", r.robot_volume_start);
        tag(out, "ConvexHullVolumeStart", r.hull_volume_start);
        tag(out, "RobotVolumeEnd", r.robot_volume_end);
        tag(out, "ConvexHullVolumeEnd", r.hull_volume_end);
        tag(out, "ShapeComplexityStart", shape_start);
        tag(out, "ShapeComplexityEnd", shape_end);
    }
    out += "    </Fitness>\n";
    if (M.vxa.variant == 0 && M.vxa.time_between_traces > 0 && M.vxa.save_traces) {     // VX_SimGA.cpp:170-184
        out += "    <CMTrace>\n";
        static const char* names[4] = {"Time", "TraceX", "TraceY", "TraceZ"};
        for (size_t i = 0; i + 3 < cm_trace.size(); i += 4) {
            out += "        <TraceStep>\n";
            for (int k = 0; k < 4; ++k) {
                char buf[64];
                std::snprintf(buf, sizeof(buf), "%g", cm_trace[i + k]);
                out += "            <"; out += names[k]; out += ">"; out += buf; out += "</"; out += names[k]; out += ">\n";
            }
            out += "        </TraceStep>\n";
        }
        out += "    </CMTrace>\n";
    }
    if (M.vxa.variant == 0 && M.vxa.norm_dist_by_vol && M.vxa.save_traces) {            // VX_SimGA.cpp:187-198
        out += "    <VolumeTrace>\n";
        for (size_t i = 0; i < vol_trace.size() && 4 * i < cm_trace.size(); ++i) {      // (SS.VolTraceTime: the times of the CoM trace)
            out += "        <TraceStep>\n";
            const double vals[2] = {cm_trace[4 * i], vol_trace[i]};
            static const char* vnames[2] = {"Time", "Volume"};
            for (int k = 0; k < 2; ++k) {
                char buf[64];
                std::snprintf(buf, sizeof(buf), "%g", vals[k]);
                out += "            <"; out += vnames[k]; out += ">"; out += buf; out += "</"; out += vnames[k]; out += ">\n";
            }
            out += "        </TraceStep>\n";
        }
        out += "    </VolumeTrace>\n";
    }
    out += "</Voxelyze_Sim_Result>\n";
    return out;
}

}  // namespace vxh
