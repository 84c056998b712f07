// Host-only check of the energy and motion stop rules (StopConditionType 4-7): what the reader accepts and what it refuses, by message.  No HIP,
// built with the plain C++ compiler (make stoprule_check), so it also runs under the host sanitizers.  Exit status 0 = all consistent.
//   stoprule_check <golden dir>     reads <golden dir>/vxa/stoprule_move2.vxa and lw_land6.vxa
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "vxa_reader.hpp"

using namespace vxh;

namespace {

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "stoprule_check: " __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

std::string slurp(const std::string& path)
{
    std::ifstream in(path, std::ios::binary);
    CHECK((bool)in, "cannot read %s", path.c_str());
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}
std::string replaced(std::string text, const std::string& from, const std::string& to)
{
    const size_t at = text.find(from);
    CHECK(at != std::string::npos && text.find(from, at + 1) == std::string::npos, "\"%s\" is not there exactly once", from.c_str());
    return text.replace(at, from.size(), to);
}
std::string with_type(const std::string& text, int from, int to)
{
    return replaced(text, "<StopConditionType>" + std::to_string(from) + "</StopConditionType>", "<StopConditionType>" + std::to_string(to) + "</StopConditionType>");
}
void expect_refused(const char* what, const std::string& text, int variant, const char* message)
{
    const VxaModel m = read_vxa(text.data(), text.size(), variant);
    bool found = false;
    for (const std::string& u : m.unsupported) found = found || u == message;
    CHECK(found, "%s: not refused with \"%s\" (%zu refusals%s%s)", what, message, m.unsupported.size(), m.unsupported.empty() ? "" : ", first: ",
          m.unsupported.empty() ? "" : m.unsupported[0].c_str());
}

}  // namespace

int main(int argc, char** argv)
{
    CHECK(argc == 2, "usage: stoprule_check <golden dir>");
    const std::string golden = argv[1];
    const std::string move2 = slurp(golden + "/vxa/stoprule_move2.vxa"), lw = slurp(golden + "/vxa/lw_land6.vxa");

    // ---- the reader: 4-7 accepted in _voxcad, 8 and above refused by value, equilibrium mode refused, land_water refused
    for (int type = 4; type <= 7; ++type) {
        const std::string t = with_type(move2, 6, type);
        const VxaModel m = read_vxa(t.data(), t.size(), 0);
        CHECK(m.unsupported.empty() && m.stop_type == type, "StopConditionType %d: not accepted", type);
    }
    expect_refused("type 8", with_type(move2, 6, 8), 0, "StopConditionType 8 (supported: 0-7)");
    expect_refused("type 12", with_type(move2, 6, 12), 0, "StopConditionType 12 (supported: 0-7)");
    expect_refused("equilibrium mode", replaced(move2, "<EquilibriumModeEnabled>0</EquilibriumModeEnabled>", "<EquilibriumModeEnabled>1</EquilibriumModeEnabled>"), 0,
                   "EquilibriumModeEnabled");
    expect_refused("land_water", with_type(lw, 2, 5), 1, "StopConditionType 5 in the land_water simulator (energy and motion stop rules: _voxcad only)");
    std::printf("reader: rules 4-7 read, four refusals: ok\n");

    return 0;
}
