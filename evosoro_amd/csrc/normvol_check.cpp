// Host-only check of <NormDistByVol> (VX_SimGA.cpp:57-112): the reader, the sums of the result file, the trace ranges of a batch.  No HIP,
// built with the plain C++ compiler (make normvol_check), so it also runs under the host sanitizers.  Exit status 0 = all consistent.
//   normvol_check <golden dir>     reads <golden dir>/vxa/normvol_{a,b,c,d}.vxa, phase4.vxa and <golden dir>/expected/normvol_*.xml
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "batch.hpp"
#include "engine.hpp"
#include "import.hpp"
#include "vxa_reader.hpp"

using namespace vxh;

namespace {

const char* g_case = "";
[[noreturn]] void fail(const char* fmt, ...)
{
    std::fprintf(stderr, "normvol_check [%s]: ", g_case);
    va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
    std::fprintf(stderr, "\n");
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

std::string slurp(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) fail("cannot read %s", path.c_str());
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

// every <tag>number</tag> of `text`, in order
std::vector<double> numbers(const std::string& text, const std::string& tag)
{
    std::vector<double> out;
    const std::string open = "<" + tag + ">";
    for (size_t at = text.find(open); at != std::string::npos; at = text.find(open, at + 1)) out.push_back(std::strtod(text.c_str() + at + open.size(), nullptr));
    return out;
}
double number(const std::string& text, const std::string& tag)
{
    const std::vector<double> all = numbers(text, tag);
    CHECK(all.size() == 1, "%zu <%s> tags", all.size(), tag.c_str());
    return all[0];
}
std::string replaced(std::string text, const std::string& from, const std::string& to)
{
    const size_t at = text.find(from);
    CHECK(at != std::string::npos && text.find(from, at + 1) == std::string::npos, "\"%s\" is not there exactly once", from.c_str());
    return text.replace(at, from.size(), to);
}

struct Fixture { const char* name; double exponent, afterlife, freeze; bool self_col; };
const Fixture FIXTURES[4] = {{"normvol_a", 1.0, 0.0, 0.0, false}, {"normvol_b", 1.5, 0.1, 0.0, false}, {"normvol_c", 1.0, 0.1, 0.1, false},
                             {"normvol_d", 1.0, 0.0, 0.0, true}};

// ---- 1. the reader: the fixtures' values; the combinations in which the reference indexes an empty vector, each with its message
void expect_refused(const char* what, const std::string& text, const char* message)
{
    const VxaModel m = read_vxa(text.data(), text.size(), 0);
    bool found = false;
    for (const std::string& u : m.unsupported) found = found || u == message;
    CHECK(found, "%s: not refused with \"%s\" (%zu refusals%s%s)", what, message, m.unsupported.size(), m.unsupported.empty() ? "" : ", first: ",
          m.unsupported.empty() ? "" : m.unsupported[0].c_str());
    try {
        read_supported_vxa(text.data(), text.size(), 0, false, "");
    } catch (const std::invalid_argument& ex) {
        CHECK(std::strstr(ex.what(), "unsupported") && std::strstr(ex.what(), message), "%s: refused with \"%s\"", what, ex.what());
        return;
    }
    fail("%s: the import accepted the file", what);
}

void check_reader(const std::string& golden)
{
    for (const Fixture& F : FIXTURES) {
        g_case = F.name;
        const std::string text = slurp(golden + "/vxa/" + F.name + ".vxa");
        const VxaModel m = read_vxa(text.data(), text.size(), 0);
        CHECK(m.unsupported.empty(), "refused: %s", m.unsupported[0].c_str());
        CHECK(m.norm_dist_by_vol, "NormDistByVol not read");
        CHECK(m.normalization_exponent == F.exponent, "NormalizationExponent %g, expected %g", m.normalization_exponent, F.exponent);
        CHECK(m.afterlife_time == F.afterlife && m.midlife_freeze_time == F.freeze, "AfterlifeTime %g, MidLifeFreezeTime %g", m.afterlife_time, m.midlife_freeze_time);
        CHECK(m.self_col_enabled == F.self_col, "SelfColEnabled %d", (int)m.self_col_enabled);
        CHECK(m.time_between_traces == 0.01 && m.save_traces && m.stop_type == 2 && m.stop_value == 0.4 && m.init_cm_time == 0.05, "trace / stop settings");
        CHECK(m.has_initial_voxel_size && m.has_final_voxel_size, "development layers");
        read_supported_vxa(text.data(), text.size(), 0, false, "");      // (throws if refused)
    }
    g_case = "refusals";
    const std::string a = slurp(golden + "/vxa/normvol_a.vxa");
    expect_refused("TimeBetweenTraces 0", replaced(a, "<TimeBetweenTraces>0.01</TimeBetweenTraces>", "<TimeBetweenTraces>0</TimeBetweenTraces>"),
                   "NormDistByVol without TimeBetweenTraces > 0");
    expect_refused("TimeBetweenTraces absent", replaced(a, "<TimeBetweenTraces>0.01</TimeBetweenTraces>", ""), "NormDistByVol without TimeBetweenTraces > 0");
    expect_refused("StopConditionType 1", replaced(a, "<StopConditionType>2</StopConditionType>", "<StopConditionType>1</StopConditionType>"),
                   "NormDistByVol with a StopConditionType other than 2 (simulation time)");
    expect_refused("StopConditionType 0", replaced(a, "<StopConditionType>2</StopConditionType>", "<StopConditionType>0</StopConditionType>"),
                   "NormDistByVol with a StopConditionType other than 2 (simulation time)");
    // what stays refused as it was
    expect_refused("NumTimeStepsInWindow", replaced(a, "<NormDistByVol>1</NormDistByVol>", "<NormDistByVol>1</NormDistByVol><NumTimeStepsInWindow>3</NumTimeStepsInWindow>"),
                   "NumTimeStepsInWindow");
    expect_refused("FallingProhibited", replaced(a, "<NormDistByVol>1</NormDistByVol>", "<NormDistByVol>1</NormDistByVol><FallingProhibited>1</FallingProhibited>"),
                   "FallingProhibited");
    // without the option the same settings are accepted as before, and the exponent defaults to 1
    const std::string off = replaced(replaced(a, "<NormDistByVol>1</NormDistByVol>", ""), "<NormalizationExponent>1.0</NormalizationExponent>", "");
    const VxaModel m = read_vxa(off.data(), off.size(), 0);
    CHECK(m.unsupported.empty() && !m.norm_dist_by_vol && m.normalization_exponent == 1.0, "the file without the option");
    const std::string off1 = replaced(off, "<StopConditionType>2</StopConditionType>", "<StopConditionType>1</StopConditionType>");
    CHECK(read_vxa(off1.data(), off1.size(), 0).unsupported.empty(), "StopConditionType 1 without the option");
    std::printf("normvol_check reader: four fixtures read, six refusals: ok\n");
}

// ---- 2. the sums.  The reference file prints its trace with six significant digits, so a sum formed from the printed points differs from the
// printed sum by what that rounding does to it.  The bound is worked out from the input alone: a printed value v stands for any number within
// |v| * 5e-6 (half a unit of the sixth digit); a term (y_i - y_{i-1}) / lat / V^e moves by at most (dy_i + dy_{i-1}) / lat / V^e for the
// y's and by |term| * e * dV / V for the volume (first order; the second-order part is below 1e-10 of it); the printed sum itself by 5e-6 of its
// magnitude, likewise the second tag where the printed one is a difference of two.
double rounding_bound(const std::vector<double>& y, const std::vector<double>& vol, double lat, double e)
{
    const double h = 5e-6;
    double bound = 0;
    for (size_t i = 1; i < y.size(); ++i) {
        const double v = (vol[i] + vol[i - 1]) / 2, term = (y[i] - y[i - 1]) / lat / std::pow(v, e);
        bound += h * (std::fabs(y[i]) + std::fabs(y[i - 1])) / lat / std::pow(v, e) + std::fabs(term) * e * h * 1.0001;
    }
    return bound;
}

void check_sums(const std::string& golden, const std::vector<RobotModel>& models)
{
    for (int f = 0; f < 4; ++f) {
        const Fixture& F = FIXTURES[f];
        g_case = F.name;
        const RobotModel& M = models[f];
        const std::string xml = slurp(golden + "/expected/" + F.name + ".xml");
        const size_t vt = xml.find("<VolumeTrace>");
        CHECK(vt != std::string::npos && xml.find("<CMTrace>") < vt, "no <VolumeTrace> behind <CMTrace>");
        const std::string cm_part = xml.substr(0, vt), vol_part = xml.substr(vt);
        const std::vector<double> t = numbers(cm_part, "Time"), x = numbers(cm_part, "TraceX"), y = numbers(cm_part, "TraceY"), z = numbers(cm_part, "TraceZ");
        const std::vector<double> tv = numbers(vol_part, "Time"), vol = numbers(vol_part, "Volume");
        CHECK(t.size() >= 30 && t.size() == y.size() && t.size() == vol.size() && t == tv, "%zu CoM points, %zu volumes", t.size(), vol.size());
        HostState S;
        S.steps = 1000; S.status = 1; S.cm_init = 1; S.cur_time = number(xml, "Lifetime") + F.afterlife; S.reduced = true;
        const double lat = M.vxa.lattice_dim, post = number(xml, "PosteriorDist");
        S.d2min = (post * lat) * (post * lat); S.d2max = S.d2min; S.ymax = S.ymin = 0;
        S.eol_post_y = number(xml, "EndOfLifePosteriorY");
        for (size_t i = 0; i < t.size(); ++i) { S.cm_trace.insert(S.cm_trace.end(), {t[i], x[i], y[i], z[i]}); S.vol_trace.push_back(vol[i]); }
        vxh_result r;
        compute_result(M, S, &r);
        const double printed_final = number(xml, "NormFinalDist"), printed_frozen = number(xml, "NormFrozenDist"), printed_regime = number(xml, "NormRegimeDist");
        // NormFinalDist is printed as final - frozen (VX_SimGA.cpp:145); the frozen trace is not in the file, so the life sum is held against
        // printed NormFinalDist + printed NormFrozenDist
        const double want = printed_final + printed_frozen;
        const double bound = rounding_bound(y, vol, lat, F.exponent) + 5e-6 * (std::fabs(printed_final) + std::fabs(printed_frozen));
        std::printf("normvol_check %s: life sum %.9g, file %.9g, difference %.3g, rounding bound %.3g\n", F.name, r.norm_final_dist, want, r.norm_final_dist - want, bound);
        CHECK(std::fabs(r.norm_final_dist - want) <= bound, "the life sum %.12g is not the file's %.12g within %.3g", r.norm_final_dist, want, bound);
        CHECK(r.norm_final_dist == norm_dist_by_vol(y.size(), y.data(), 1, vol.data(), 1, lat, F.exponent), "compute_result does not use norm_dist_by_vol");
        // no frozen / after-life points handed over: the defined 0 where the reference reads element [0] of an empty vector
        CHECK(r.norm_frozen_dist == 0, "NormFrozenDist %g from an empty frozen trace", r.norm_frozen_dist);
        if (F.afterlife > 0) CHECK(r.norm_regime_dist == 0, "NormRegimeDist %g from an empty after-life trace", r.norm_regime_dist);
        else {
            // without AfterlifeTime the tag stays the posterior-edge difference (VX_SimGA.cpp:38), here from the printed tags: each within 5e-6 of itself
            const double rb = 5e-6 * (std::fabs(post) + std::fabs(S.eol_post_y) + std::fabs(printed_regime)) * 1.0001;
            CHECK(std::fabs(r.norm_regime_dist - printed_regime) <= rb, "NormRegimeDist %.9g, file %.9g", r.norm_regime_dist, printed_regime);
            CHECK(printed_frozen == 0, "NormFrozenDist %g without a freeze", printed_frozen);
        }
        // the frozen and after-life sums take the same route: the life trace's points handed over as those traces give the life sum, bit for bit
        for (size_t i = 0; i < t.size(); ++i)
            for (int w = 0; w < 2; ++w) S.xtrace[w].insert(S.xtrace[w].end(), {t[i], x[i], y[i], z[i], vol[i]});
        compute_result(M, S, &r);
        if (F.afterlife > 0) CHECK(r.norm_regime_dist == r.norm_final_dist, "the after-life sum takes another route");
        if (F.freeze > 0) CHECK(r.norm_frozen_dist == r.norm_final_dist, "the frozen sum takes another route");
        else CHECK(r.norm_frozen_dist == 0, "a frozen sum without MidLifeFreezeTime");
        // the XML: <VolumeTrace> behind <CMTrace>, the reference's structure tag for tag, and its text where the numbers are the file's own
        const std::string ours = result_xml(M, r, S.cm_trace, -1.0, -1.0, S.vol_trace);
        const size_t vo = ours.find("<VolumeTrace>");
        CHECK(vo != std::string::npos, "no <VolumeTrace> in the result file");
        CHECK(ours.substr(ours.find("<CMTrace>")) == xml.substr(xml.find("<CMTrace>")), "the trace blocks are not the reference's text");
    }
    // fewer than two points: 0
    g_case = "short traces";
    const double y2[2] = {1.0, 3.0}, v2[2] = {2.0, 6.0};
    CHECK(norm_dist_by_vol(0, y2, 1, v2, 1, 0.5, 1.0) == 0 && norm_dist_by_vol(1, y2, 1, v2, 1, 0.5, 1.0) == 0, "a trace of fewer than two points");
    CHECK(norm_dist_by_vol(2, y2, 1, v2, 1, 0.5, 2.0) == (3.0 - 1.0) / 0.5 / std::pow(4.0, 2.0), "a trace of two points");
    std::printf("normvol_check sums: four reference files reproduced: ok\n");
}

// ---- 3. assemble_batch: three trace ranges for a robot with the option, none of the new ones for a robot without
void check_ranges(const std::vector<RobotModel>& models)
{
    g_case = "ranges";
    const HostBatch H = assemble_batch(models, 0, Options(), 0);
    const int nr = (int)models.size();
    int vol = 0, xt = 0;
    for (int r = 0; r < nr; ++r) {
        const VxaModel& X = models[r].vxa;
        const DRobot& R = H.robot[r];
        CHECK(R.vol_begin == vol && H.vol_begin[r] == vol, "robot %d: volumes begin at %d, expected %d", r, R.vol_begin, vol);
        if (!X.norm_dist_by_vol) {
            CHECK(!(R.flags & RF_NORM_VOL) && R.xt_cap[0] == 0 && R.xt_cap[1] == 0, "robot %d has no option but flags %d, ranges %d %d", r, R.flags, R.xt_cap[0], R.xt_cap[1]);
            continue;
        }
        CHECK((R.flags & RF_NORM_VOL) && R.trace_cap > 0 && R.trace_dt == X.time_between_traces, "robot %d: flag or life trace missing", r);
        // every point UpdateStats can record fits: the life trace after InitCmTime, the others within AfterlifeTime / MidLifeFreezeTime (+ the step that crosses the end)
        const double total = (double)models[r].planned_steps * models[r].dt;
        CHECK(R.trace_cap >= (total - X.init_cm_time) / X.time_between_traces + 2, "robot %d: life trace of %d entries", r, R.trace_cap);
        vol += R.trace_cap;
        const double span[2] = {X.afterlife_time, X.midlife_freeze_time};
        for (int k = 0; k < 2; ++k) {
            CHECK(R.xt_begin[k] == xt && H.xt_begin[k][r] == xt, "robot %d trace %d begins at %d, expected %d", r, k + 1, R.xt_begin[k], xt);
            if (span[k] > 0) CHECK(R.xt_cap[k] >= span[k] / X.time_between_traces + 2 && R.xt_cap[k] <= span[k] / X.time_between_traces + 8, "robot %d trace %d: %d entries", r, k + 1, R.xt_cap[k]);
            else CHECK(R.xt_cap[k] == 0, "robot %d trace %d: %d entries without its span", r, k + 1, R.xt_cap[k]);
            CHECK(R.xt_cap[k] == H.xt_cap[k][r], "robot %d trace %d: DRobot and HostBatch differ", r, k + 1);
            xt += R.xt_cap[k];
        }
        CHECK(H.rstate[r].nxtrace[0] == 0 && H.rstate[r].nxtrace[1] == 0, "robot %d starts with trace points", r);
    }
    CHECK(H.total_vol == vol && H.total_xtrace == xt, "totals %d %d, expected %d %d", H.total_vol, H.total_xtrace, vol, xt);
    CHECK(vol > 0 && xt > 0, "no ranges at all");
    std::printf("normvol_check ranges: %d robots, %d volumes, %d after-life / frozen entries: ok\n", nr, vol, xt);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: normvol_check <golden dir>\n"); return 2; }
    const std::string golden = argv[1];
    check_reader(golden);
    std::vector<std::string> paths;
    for (const Fixture& F : FIXTURES) paths.push_back(golden + "/vxa/" + F.name + ".vxa");
    paths.push_back(golden + "/vxa/phase4.vxa");           // a robot without the option
    const std::vector<RobotModel> models = build_vxa_files(paths, 0, false);
    check_sums(golden, models);
    check_ranges(models);
    return 0;
}
