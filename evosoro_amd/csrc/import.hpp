// Import pipeline, plain C++ (no HIP): .vxa text, .vxa files or a generation handed over as arrays -> robot models.  Parses and builds (may
// throw, touches no engine); Engine::append takes what it returns.  `want_mesh`: the engine's option shape_descriptors.
#pragma once
#include <algorithm>
#include <atomic>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vxhip.h"
#include "model.hpp"

namespace vxh {

// body(i) for every i in [0, n), spread over min(n, max_threads, host cores) threads that draw indices from one counter; the caller
// works as the first of them.  Every index is attempted; the first failure IN INDEX ORDER is rethrown after the join.
template <class Body>
void for_each_index(int n, int max_threads, Body&& body)
{
    std::vector<std::exception_ptr> errors(std::max(n, 0));
    std::atomic<int> next{0};
    auto worker = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            try { body(i); } catch (...) { errors[i] = std::current_exception(); }
        }
    };
    const int nthreads = std::max(1, std::min({n, max_threads, (int)std::thread::hardware_concurrency()}));
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    for (const auto& e : errors) if (e) std::rethrow_exception(e);
}

// read_vxa + want_mesh; features the engine does not model are refused: std::invalid_argument("unsupported .vxa feature(s): [a] [b]" + where),
// where = "", " in <path>" or " in the template" (the C ABI maps the word "unsupported" to VXH_ERR_UNSUPPORTED)
VxaModel read_supported_vxa(const char* data, size_t len, int variant, bool want_mesh, const std::string& where);

std::vector<RobotModel> build_vxa(const char* data, size_t len, int variant, bool want_mesh);
std::vector<RobotModel> build_vxa_files(const std::vector<std::string>& paths, int variant, bool want_mesh);   // in the order of `paths`
// A generation handed over as arrays (vxh_add_robots), in two steps: the cheap one (template parse, argument checks, the arrays copied
// into .vxa models: everything that can be REFUSED) and the expensive one (model building).  A handle that pipelines a generation does
// the first when the robots are added and the second chunk by chunk while earlier chunks already step (EngineSet::run).
std::vector<VxaModel> models_from_arrays(const char* template_vxa, size_t len, const vxh_robot_arrays* robots, int n, bool round_like_text, int variant, bool want_mesh);
std::vector<RobotModel> build_models(std::vector<VxaModel>&& models);
std::vector<RobotModel> build_arrays(const char* template_vxa, size_t len, const vxh_robot_arrays* robots, int n, bool round_like_text, int variant, bool want_mesh);

}  // namespace vxh
