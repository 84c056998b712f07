// Engine implementation: HBM upload, step-round launches (hipGraph), download.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>

#include "batch.hpp"
#include "engine.hpp"
#include "import.hpp"
#include "dev_report.hpp"
#include "device_types.hpp"
#include "launch.hpp"

namespace vxh {

#define HIP_OK(call) hip_check((call), #call)

int hip_device_count()
{
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

struct Engine::Device {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // fused path: robots grouped by kernel variant (workgroup size 256/512/768/1024, exchange buffers, fluid), one
    // stream per group so that the groups fill the chip together
    struct Group : GroupPlan {            // (batch.hpp: the kernel variant, its robots sorted, LDS bytes) + the HIP side
        explicit Group(GroupPlan&& p) : GroupPlan(std::move(p)) {}
        const int* list = nullptr;
        // dispatch order of short launches (kernels_fused.hpp fused_dispatch_slot): one bit per list entry, written by a launch for the next
        unsigned long long* order_bits[2] = {nullptr, nullptr};
        int order_cur = 0;
        bool order_valid = false;
        // ... and of long ones (dispatch_order.hpp): the permutation k_dispatch_order makes for a launch, and behind it what every workgroup
        // of the last long launch measured its robot to cost, by list entry.  The ordering kernel and the launches of a group follow each
        // other on one stream: one buffer.  No long launch yet (a new batch, a reset): no measurement, the list order.
        int* order_perm = nullptr;
        bool cost_valid = false;          // a long launch has left cost words
        bool last_ordered = false;        // (VXH_PROF_ORDER: the last long launch was ordered by cost; its length)
        long long last_len = 0;
        hipStream_t stream = nullptr;
        hipEvent_t t0 = nullptr, t1 = nullptr;
    };
    std::vector<Group> groups;
    std::vector<hipStream_t> group_streams;   // created on demand, reused across prepare() calls
    std::vector<hipEvent_t> group_events;
    void give_stream(Group& g, size_t gi)     // the gi-th group of a batch: its stream and events
    {
        if (group_streams.size() <= gi) {
            hipStream_t st; hipEvent_t e0, e1;
            // launch groups of one call are meant to run side by side (two size classes of one population: 64 + 64 workgroups on 256
            // CUs).  Streams share a few hardware queues, handed out round robin as streams are created: two group streams that
            // land on the same queue run their kernels one after the other (measured: the same 64 robots of two size classes
            // 14.8 or 24.3 us per step, depending on how many streams the process had created before).  Streams of different
            // priority never share a queue, so the group streams cycle through the priorities the device offers.
            int least = 0, greatest = 0;
            HIP_OK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            const int span = least - greatest + 1;                 // (numerically: greatest priority = smallest number)
            const int prio = span > 1 ? greatest + (int)(group_streams.size() % (size_t)span) : 0;
            HIP_OK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
            HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
            group_streams.push_back(st); group_events.push_back(e0); group_events.push_back(e1);
        }
        g.stream = group_streams[gi]; g.t0 = group_events[2 * gi]; g.t1 = group_events[2 * gi + 1];
    }
    const unsigned char* streamed_all = nullptr;    // masks for DBatch::streamed: every robot / the robots outside the launch groups
    const unsigned char* streamed_rest = nullptr;
    int n_rest = 0, n_all = 0;            // robots (with voxels) that only the streaming kernels can step / that they step with fused = 0
    const unsigned char* graph_mask = nullptr;      // the mask the captured graph was recorded with
    bool any_fluid = false;               // some robot is in a fluid: the streaming rounds include the drag kernels
    std::vector<void*> allocs;
    DBatch B{};
    std::vector<DRobot> h_robot;
    std::vector<int> vox_begin;           // per robot, global slot of voxel 0
    std::vector<int> trace_begin, trace_cap;   // per robot, entries of DBatch::trace
    int total_trace = 0;
    std::vector<int> vol_begin, xt_begin[2], xt_cap[2];   // robots with <NormDistByVol>: entries of DBatch::trace_vol / xtrace (HostBatch)
    int total_vol = 0, total_xtrace = 0;
    std::vector<int> surf_begin;
    int total_surf = 0;
    long long max_planned = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_rounds = 0;
    int max_nvox = 0;                     // largest robot of the batch (selects the fused block size)
    // tiled path: the robots cut into tiles, packed into launches that fit the chip (all tiles of a robot in one launch)
    struct TileLaunch : TileLaunchPlan {  // (batch.hpp: the kernel variant, tile ids, robots, LDS bytes)
        explicit TileLaunch(TileLaunchPlan&& p) : TileLaunchPlan(std::move(p)) {}
        const int* list = nullptr;        // tile ids
    };
    std::vector<TileLaunch> tile_launches;
    std::vector<unsigned char> robot_tiled;   // per robot
    std::vector<int> robot_tiles;             // per robot: number of tiles (0 = not tiled)
    hipStream_t tile_stream = nullptr;        // ONE stream for every tiled launch: two of them must never share the chip
    hipEvent_t tile_t0 = nullptr, tile_t1 = nullptr;
    int n_cu = 0;
    DResult* results = nullptr;               // [robots] output of k_results (freed with the batch)
    DRobotState* h_rstate = nullptr;          // pinned host mirror of DBatch::rstate: copied back on the call's own stream, behind its kernels
    size_t h_rstate_cap = 0;
    // a call that has been launched and not yet waited for (advance_launch / advance_finish)
    struct Pending {
        bool active = false;
        long long todo = 0, launches = 0, tile_launch_count = 0;
        bool fused = false, tiled = false, streaming = false, single = false;
        std::vector<int> steps_before;
        std::vector<long long> group_launches;
    } pending;
    int reb_blocks = 0;                   // streaming path: collision-rebuild blocks appended to k_bonds
    const int* reb_robot = nullptr;
    const int* reb_i0 = nullptr;

    // Allocations and uploads go through the engine's own stream (stream-ordered pool): hipMalloc / hipMemcpy / hipFree synchronise
    // with the whole device, and a handle that pipelines a generation prepares chunk k + 1 while the kernels of chunk k run --
    // measured: "allocations + uploads" of the second chunk 6 ms alone, 38 ms next to a running kernel with the synchronous calls.
    // The host vectors are pageable: hipMemcpyAsync returns once it has staged them; prepare() ends with a wait for this stream.
    bool async_alloc = std::getenv("VXH_SYNC_ALLOC") == nullptr;
    bool dbg_alloc = std::getenv("VXH_DBG_ALLOC") != nullptr;
    std::vector<size_t> alloc_bytes;
    std::vector<std::pair<void*, std::vector<char>>> dbg_uploads;      // (VXH_DBG_ALLOC: what every upload sent, for verify_uploads)
    void verify_uploads(const char* when)
    {
        if (!dbg_alloc) return;
        int n_bad = 0;
        for (size_t k = 0; k < dbg_uploads.size(); ++k) {
            std::vector<char> back(dbg_uploads[k].second.size());
            if (hipMemcpy(back.data(), dbg_uploads[k].first, back.size(), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "vxhip: VERIFY %s: read-back of upload #%zu failed\n", when, k); continue; }
            size_t first = back.size(), count = 0, zeros = 0;
            for (size_t i = 0; i < back.size(); ++i) if (back[i] != dbg_uploads[k].second[i]) { if (first == back.size()) first = i; ++count; zeros += back[i] == 0; }
            if (count) { ++n_bad; std::fprintf(stderr, "vxhip: VERIFY %s: upload #%zu at %p (%zu bytes) differs in %zu bytes from offset %zu on (%zu of them read 0)\n", when, k, dbg_uploads[k].first, back.size(), count, first, zeros); }
        }
        std::fprintf(stderr, "vxhip: VERIFY %s: %d of %zu uploads differ\n", when, n_bad, dbg_uploads.size());
    }
    void* raw_alloc(size_t bytes)
    {
        void* p = nullptr;
        if (async_alloc) HIP_OK(hipMallocAsync(&p, bytes, stream)); else HIP_OK(hipMalloc(&p, bytes));
        if (dbg_alloc) {
            for (size_t k = 0; k < allocs.size(); ++k)
                if ((char*)p < (char*)allocs[k] + alloc_bytes[k] && (char*)allocs[k] < (char*)p + bytes)
                    std::fprintf(stderr, "vxhip: ALLOCATION OVERLAP: new %p + %zu against live #%zu %p + %zu\n", p, bytes, k, allocs[k], alloc_bytes[k]);
            alloc_bytes.push_back(bytes);
        }
        allocs.push_back(p);
        return p;
    }
    template <class T>
    T* upload(const std::vector<T>& h, size_t min_count = 1)
    {
        size_t n = std::max(h.size(), min_count);
        void* p = raw_alloc(n * sizeof(T));
        if (!h.empty()) {
            if (async_alloc) HIP_OK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
            else HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
            if (dbg_alloc) dbg_uploads.emplace_back(p, std::vector<char>((const char*)h.data(), (const char*)h.data() + h.size() * sizeof(T)));
        }
        return (T*)p;
    }
    template <class T>
    T* alloc_zero(size_t n)
    {
        if (n == 0) n = 1;
        void* p = raw_alloc(n * sizeof(T));
        if (async_alloc) HIP_OK(hipMemsetAsync(p, 0, n * sizeof(T), stream)); else HIP_OK(hipMemset(p, 0, n * sizeof(T)));
        return (T*)p;
    }
    template <class T>
    T* alloc_raw(size_t n)
    {
        if (n == 0) n = 1;
        return (T*)raw_alloc(n * sizeof(T));
    }
    // every stream of this engine idle, no sticky error: the state a failed call must leave behind, and what freeing a batch waits for
    void idle()
    {
        for (hipStream_t st : group_streams) (void)hipStreamSynchronize(st);
        if (tile_stream) (void)hipStreamSynchronize(tile_stream);
        if (stream) (void)hipStreamSynchronize(stream);
        (void)hipGetLastError();
    }
    void drop_graph()
    {
        if (graph_exec) { hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
        if (graph) { hipGraphDestroy(graph); graph = nullptr; }
    }
    // (the allocations are freed in the order of `stream` alone, their consumers ran on the group and tile streams too: idle() first)
    void free_all()
    {
        if (!allocs.empty()) idle();
        if (h_rstate) { hipHostFree(h_rstate); h_rstate = nullptr; h_rstate_cap = 0; }
        drop_graph();
        if (async_alloc && stream) { for (void* p : allocs) hipFreeAsync(p, stream); if (!allocs.empty()) hipStreamSynchronize(stream); }
        else for (void* p : allocs) hipFree(p);
        allocs.clear();
        alloc_bytes.clear();
        dbg_uploads.clear();
        results = nullptr;
        B = DBatch{};
    }
    ~Device()                             // (the owner has made the device current)
    {
        free_all();
        for (hipEvent_t ev : {ev0, ev1, tile_t0, tile_t1}) if (ev) hipEventDestroy(ev);
        for (hipStream_t st : {stream, tile_stream}) if (st) hipStreamDestroy(st);
        for (hipStream_t st : group_streams) hipStreamDestroy(st);
        for (hipEvent_t ev : group_events) hipEventDestroy(ev);
    }
    void report_dispatch_cost();          // VXH_PROF_ORDER=1: what the robots of the last launch of every group cost, on stderr
#ifdef VXH_PHASE_TIMING
    void report_contact_rows(const std::vector<RobotModel>& robots);      // the developer build's report of a batch (Engine::clear)
    void report_phase_counters();
#endif
};

Engine::Engine(int variant, int device_id) : variant_(variant), device_id_(device_id), dev_(new Device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        throw std::runtime_error("no HIP device available (libvxhip has no CPU path)");
    if (device_id < 0 || device_id >= count) throw std::runtime_error("device id out of range");
    HIP_OK(hipSetDevice(device_id));
    // The stream-ordered pool keeps what the engines free (release threshold: everything) instead of handing it back to the driver at every
    // synchronisation.  Round 6, found by looping the GPU tests: a call that failed halfway (a refused tile kernel), then reset() -- free,
    // release, acquire again, upload -- left the FIRST TWO uploads of the new batch (DRobot and DRobotState, the first 0x290 bytes of the
    // re-acquired chunk) zeroed in 3 % of fresh processes: correct right behind their copies, zero at the end of prepare() (VXH_DBG_ALLOC=1
    // reads every upload back), i.e. cleared by something that is not the engine's; never with hipMalloc (VXH_SYNC_ALLOC), never with the
    // memory kept (0 of 250 against 7-8 of 250; gpurun_out/r6/refusedloop*.txt, HISTORY "Round 6").  A population's footprint is what the
    // process needed at its peak anyway, and re-mapping it every generation costs time.  VXH_POOL_RELEASE=1: the runtime's default back.
    if (!std::getenv("VXH_POOL_RELEASE")) {
        hipMemPool_t pool = nullptr;
        if (hipDeviceGetDefaultMemPool(&pool, device_id) == hipSuccess && pool) {
            uint64_t keep = ~0ull;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        (void)hipGetLastError();
    }
    HIP_OK(hipStreamCreateWithFlags(&dev_->stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&dev_->ev0));
    HIP_OK(hipEventCreate(&dev_->ev1));
    HIP_OK(hipStreamCreateWithFlags(&dev_->tile_stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&dev_->tile_t0));
    HIP_OK(hipEventCreate(&dev_->tile_t1));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device_id));
    dev_->n_cu = prop.multiProcessorCount;
    // VXH_ENGINE_OPTIONS="key=value,key=value": defaults of vxh_set_option for every engine of the process, so that a caller
    // that cannot pass options (the voxelyze command line, a test matrix) still selects e.g. tiled=0
    if (const char* env = std::getenv("VXH_ENGINE_OPTIONS")) {
        std::stringstream list(env);
        std::string item;
        while (std::getline(list, item, ',')) {
            const size_t eq = item.find('=');
            if (eq == std::string::npos || eq == 0) throw std::runtime_error("VXH_ENGINE_OPTIONS: expected key=value, got '" + item + "'");
            set_option(item.substr(0, eq), std::stod(item.substr(eq + 1)));
        }
    }
}

Engine::~Engine() { if (dev_) hipSetDevice(device_id_); }      // (~Device frees the batch, the streams and the events)

// The add_* calls are the build_* functions of import.hpp (parse + model building: may throw, touch nothing) followed by append(): a
// refused call leaves the engine -- and, behind a handle over several devices, the distribution of the robots -- as it was.
int Engine::append(std::vector<RobotModel>&& built)
{
    const int first = (int)robots_.size();
    for (auto& m : built) robots_.push_back(std::move(m));
    prepared_ = false;
    state_downloaded_ = control_downloaded_ = reduced_downloaded_ = false;
    return first;
}
int Engine::add_vxa(const char* data, size_t len) { return append(build_vxa(data, len, variant_, wants_mesh())); }
int Engine::add_vxa_files(const std::vector<std::string>& paths) { return append(build_vxa_files(paths, variant_, wants_mesh())); }
int Engine::add_arrays(const char* template_vxa, size_t len, const vxh_robot_arrays* in, int n, bool round_like_text)
{ return append(build_arrays(template_vxa, len, in, n, round_like_text, variant_, wants_mesh())); }

// no batch prepared, nothing downloaded, no step taken (the robots stay)
void Engine::forget_batch()
{
    host_.clear();
    prepared_ = state_downloaded_ = control_downloaded_ = reduced_downloaded_ = false;
    rounds_done_ = 0;
}

std::vector<RobotModel> Engine::take_robots()
{
    HIP_OK(hipSetDevice(device_id_));
    dev_->free_all();
    std::vector<RobotModel> out = std::move(robots_);
    robots_.clear();
    forget_batch();
    return out;
}

void Engine::set_tiling_allowed(bool on)
{
    if (on == tiling_allowed_) return;
    if (prepared_ && rounds_done_ > 0) throw std::logic_error("the kernel choice of a batch that has stepped cannot change");
    tiling_allowed_ = on;
    prepared_ = false;
}

// VXH_PROF_ORDER=1, after every call: what the robots cost in the last LONG launch of every colliding k_robot_steps group (dev_report.cpp)
void Engine::Device::report_dispatch_cost()
{
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0) != hipSuccess || khz <= 0) khz = 100000;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        if (!g.order_perm || !g.cost_valid) continue;
        std::vector<DispatchCost> c(g.count);
        std::vector<int> perm(g.count);
        HIP_OK(hipMemcpy(c.data(), order_ws_cost(g.order_perm, g.count), sizeof(DispatchCost) * c.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < g.count; ++k) perm[k] = k;
        if (g.last_ordered) HIP_OK(hipMemcpy(perm.data(), g.order_perm, sizeof(int) * perm.size(), hipMemcpyDeviceToHost));
        vxh::report_dispatch_cost(gi, c, perm, g.block, g.lds, g.last_len, g.last_ordered, n_cu, 1e3 / (double)khz);
    }
}

#ifdef VXH_PHASE_TIMING
// The developer build's report of a batch that is about to go (dev_report.cpp)
void Engine::Device::report_contact_rows(const std::vector<RobotModel>& robots)
{
    if (!std::getenv("VXH_COL_STATS") || B.col_rows <= 0) return;    // lengths of the contact rows as the last broad-phase runs left them
    std::vector<int> cnt(B.col_rows), nsurf;
    HIP_OK(hipMemcpy(cnt.data(), B.col_cnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
    for (const RobotModel& m : robots) nsurf.push_back(m.nsurf);
    vxh::report_contact_rows(cnt, surf_begin, nsurf);
}

void Engine::Device::report_phase_counters()
{
    if (!B.prof) return;
    std::vector<unsigned long long> h(VXH_PROF_WORDS);
    HIP_OK(hipMemcpy(h.data(), B.prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    vxh::report_phase_counters(h.data(), B.n_tiles, !tile_launches.empty());
}
#endif

void Engine::clear()
{
#ifdef VXH_PHASE_TIMING
    HIP_OK(hipSetDevice(device_id_));
    dev_->report_contact_rows(robots_);
    dev_->report_phase_counters();
#endif
    take_robots();
}

// A captured step graph holds the kernel arguments (the whole DBatch, by value) of the moment it was captured: every option that
// changes one of them, or which kernels a round consists of, drops it; the next graph-sized call captures afresh.
void Engine::drop_graph()
{
    HIP_OK(hipSetDevice(device_id_));
    dev_->drop_graph();
}

// The options of vxh_set_option, each described once.  A FLAG is stored as value != 0, an INT truncated.  Accepted values: ANY, the WHOLE
// numbers lo..hi, or the RANGE lo <= value <= hi.  `batch`: which kernel steps a robot, its tiling and the size of its contact rows are
// part of the uploaded batch -- set before the first vxh_run / vxh_step, or right after vxh_reset (no step taken yet: the batch is then
// assembled again at the next run); an unchanged value is always fine, nothing would be assembled again.  (`fused` too, since round 5:
// the resident kernels keep the bond history in their own array and a saved image of the contact rows, so a robot that changed kernels
// in the middle of a run would read stale history -- ADVICE round 4.)  `graph`: the captured step graph depends on it (drop_graph).
namespace {
struct OptionDesc {
    const char* name;
    int Options::*member;
    enum Kind { FLAG, INT } kind;
    enum Accept { ANY, WHOLE, RANGE } accept;
    double lo, hi;
    bool batch, graph;
    int coerce(double value) const { return kind == FLAG ? (int)(value != 0) : (int)value; }
    bool accepts(double value) const { return accept == ANY || (value >= lo && value <= hi && (accept == RANGE || value == std::trunc(value))); }
};
const OptionDesc option_table[] = {
    {"tiled",             &Options::tiled,             OptionDesc::INT,  OptionDesc::WHOLE, 0, 2,      true,  false},
    {"tiles_per_robot",   &Options::tiles_per_robot,   OptionDesc::INT,  OptionDesc::RANGE, 0, 4096,   true,  false},
    {"tile_small",        &Options::tile_small,        OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      true,  false},
    {"wide",              &Options::wide,              OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      true,  false},
    {"wide_two_tiles",    &Options::wide_two_tiles,    OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      true,  false},
    {"col_cap",           &Options::col_cap,           OptionDesc::INT,  OptionDesc::RANGE, 0, 1e6,    true,  false},
    {"fused",             &Options::fused,             OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      true,  true},
    {"steps_per_launch",  &Options::steps_per_launch,  OptionDesc::INT,  OptionDesc::RANGE, 1, 200000, false, false},
    {"graph_steps",       &Options::graph_steps,       OptionDesc::INT,  OptionDesc::RANGE, 0, 1e6,    false, true},
    {"shape_descriptors", &Options::shape_descriptors, OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      false, false},      // (robots added FROM NOW ON carry the surface mesh)
    {"host_results",      &Options::host_results,      OptionDesc::FLAG, OptionDesc::ANY,   0, 0,      false, false},
    {"dispatch_order",    &Options::dispatch_order,    OptionDesc::FLAG, OptionDesc::WHOLE, 0, 1,      false, false},
};
const OptionDesc& find_option(const std::string& key)
{
    for (const OptionDesc& d : option_table) if (key == d.name) return d;
    throw std::invalid_argument("unknown option " + key);
}
}  // namespace

// throws what set_option would throw for this key / value in the engine's present state, and changes nothing: a handle over several
// devices applies an option to all of its engines or to none
void Engine::check_option(const std::string& key, double value) const
{
#ifdef VXH_PHASE_TIMING
    if (key == "dbg") return;                 // physics-skipping what-if switches: developer library only
#endif
    const OptionDesc& d = find_option(key);
    if (d.batch && prepared_ && rounds_done_ > 0 && opt_.*d.member != d.coerce(value))      // (the state of the batch is judged before the value)
        throw std::logic_error("option " + key + " must be set before the first vxh_run/vxh_step (or right after vxh_reset)");
    if (!d.accepts(value)) {
        char want[64];
        std::snprintf(want, sizeof(want), d.accept == OptionDesc::WHOLE ? ": a whole number from %g to %g" : ": %g to %g", d.lo, d.hi);
        throw std::invalid_argument(key + want);
    }
}

void Engine::set_option(const std::string& key, double value)
{
    check_option(key, value);
#ifdef VXH_PHASE_TIMING
    if (key == "dbg") { dbg_ = (int)value; dev_->B.dbg = dbg_; drop_graph(); return; }
#endif
    const OptionDesc& d = find_option(key);
    const int want = d.coerce(value);
    if (d.batch) {
        if (opt_.*d.member == want) return;   // (unchanged: the assembled batch stays)
        prepared_ = false;                    // (the batch is assembled again at the next run)
    }
    opt_.*d.member = want;
    if (d.graph) drop_graph();
    if (d.member == &Options::host_results) reduced_downloaded_ = false;
}

// where the host-side time of a run goes (VXH_PROF_HOST=1: one line per prepare() / advance() on stderr)
namespace {
struct HostStages {
    const bool on = std::getenv("VXH_PROF_HOST") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    std::string line;
    void mark(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96]; std::snprintf(buf, sizeof(buf), " %s %.3f ms |", what, 1e3 * std::chrono::duration<double>(now - t).count());
        line += buf; t = now;
    }
    void print(const char* head) { if (on) std::fprintf(stderr, "%s:%s\n", head, line.c_str()); }
};
}

// Build + upload the batch.  The host tables (assemble_batch) and the tiling / launch groups (plan_launches) are worked out in batch.cpp;
// the plan is made while the uploads of the tables drain.  Allocations and uploads keep their order: the stream-ordered pool hands out
// addresses in call order.
void Engine::prepare()
{
    HostStages hs;
    HIP_OK(hipSetDevice(device_id_));
    Device& D = *dev_;
    D.free_all();
    hs.mark("free");
    const int nr = (int)robots_.size();
    size_t free_b = 0, total_b = 0;           // (the contact-row budget; only asked for when no col_cap bounds the rows)
    if (opt_.col_cap <= 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
    HostBatch H = assemble_batch(robots_, variant_, opt_, total_b);
    const int nv = H.nv, ns = H.ns;
    hs.mark("host assembly");
    DBatch& B = D.B;
    B.n_robots = nr; B.nv = nv; B.dbg = dbg_;
    B.robot = D.upload(H.robot);
    B.rstate = D.upload(H.rstate);
    {   // ... and their mirror in pinned host memory, which the resident kernels write as well (a call that runs one launch group and
        // nothing else needs no copy back: ~10-15 us of a 0.7 ms call); start values for the robots no kernel touches
        if (D.h_rstate_cap < (size_t)nr) {
            if (D.h_rstate) HIP_OK(hipHostFree(D.h_rstate));
            D.h_rstate = nullptr; D.h_rstate_cap = 0;
            HIP_OK(hipHostMalloc((void**)&D.h_rstate, sizeof(DRobotState) * std::max(nr, 1), hipHostMallocDefault));
            D.h_rstate_cap = (size_t)std::max(nr, 1);
        }
        std::memcpy(D.h_rstate, H.rstate.data(), sizeof(DRobotState) * nr);
        void* dp = nullptr;
        B.rstate_mirror = hipHostGetDevicePointer(&dp, D.h_rstate, 0) == hipSuccess ? (DRobotState*)dp : nullptr;
    }
    B.wave_robot = D.upload(H.wave_robot);
    B.vclass_tab = D.upload(H.vtab);
    B.bclass_tab = D.upload(H.btab);
    B.vclass = D.upload(H.vclass);
    B.bclass = D.upload(H.bclass);
    B.nbr = D.upload(H.nbr);
    B.bsched = D.upload(H.bsched);
    B.wlist = D.upload(H.wlist);
    B.wgather = D.upload(H.wgather);
    B.act_sb = D.upload(H.act_sb);
    B.act_cb = D.upload(H.act_cb);
    B.amp_damp = D.upload(H.amp_damp);
    B.dev = D.upload(H.dev);
    {   // vs[18][nv]: nominal position + scale in both buffers, identity quaternions, zero momenta
        double* vs = D.alloc_zero<double>((size_t)18 * nv);
        const std::vector<double>* planes[5] = {&H.px, &H.py, &H.pz, &H.sc, &H.qw};
        for (int k = 0; k < 5; ++k)
            HIP_OK(hipMemcpyAsync(vs + (size_t)(k < 4 ? k : 8) * nv, planes[k]->data(), sizeof(double) * nv, hipMemcpyHostToDevice, D.stream));
        HIP_OK(hipMemcpyAsync(vs + (size_t)4 * nv, vs, sizeof(double) * 4 * nv, hipMemcpyDeviceToDevice, D.stream));
        B.vs = vs;
    }
    B.hist = D.alloc_zero<double>((size_t)6 * 3 * nv);
    B.hist_aos = D.alloc_zero<double>((size_t)6 * 3 * nv);
    B.small_angle = D.upload(H.small);
    B.bout = D.alloc_zero<double>((size_t)12 * 3 * nv);
    B.surf = D.upload(H.surf);
    B.surf_code = D.upload(H.surf_code);
    B.surf_ord = D.upload(H.surf_ord);
    B.excl = D.upload(H.excl);
    B.total_mv = std::max(H.total_mv, 1);
    B.vert_pack = D.upload(H.vert_pack);
    B.vert_v0 = D.upload(H.vert_v0);
    B.total_facet = std::max(H.total_facet, 1);
    B.facet_vox = D.upload(H.facet_vox);
    B.facet_vert = D.upload(H.facet_vert);
    B.facet_first = D.upload(H.facet_first);
    B.facet_count = D.upload(H.facet_count);
    B.strain = D.alloc_zero<double>(H.any_mesh ? (size_t)6 * nv : 1);
    B.n_mv = H.total_mv; B.n_facet = H.total_facet;
    B.vert_vox = D.upload(H.vert_vox);
    B.vert_robot = D.upload(H.vert_robot);
    B.facet_robot = D.upload(H.facet_robot);
    B.mesh_pos = D.alloc_zero<double>(H.any_fluid ? (size_t)3 * std::max(H.total_mv, 1) : 1);
    B.fdrag = D.alloc_zero<double>(H.any_fluid ? (size_t)3 * std::max(H.total_facet, 1) : 1);
    D.any_fluid = H.any_fluid;
    B.trace = D.alloc_zero<double>((size_t)std::max(H.total_trace, 1) * 4);
    B.trace_vol = D.alloc_zero<double>((size_t)std::max(H.total_vol, 1));
    B.xtrace = D.alloc_zero<double>((size_t)std::max(H.total_xtrace, 1) * 5);
    B.col_rows = std::max(ns, 1);
    B.col_cnt = D.alloc_zero<int>(std::max(ns, 1));
    {   // saved LDS images of the contact rows (resident kernel): one slot per colliding robot of up to 1024 voxels
        int n_img = 0;
        for (int r = 0; r < nr; ++r) if (H.img_idx[r] >= 0) ++n_img;
        B.rimg_code = D.alloc_raw<int>((size_t)std::max(n_img, 1) * VXH_RIMG_CAP);
        B.rimg_a1 = D.alloc_raw<double>((size_t)std::max(n_img, 1) * VXH_RIMG_CAP);
        B.rimg_seg = D.alloc_zero<int>((size_t)std::max(n_img, 1) * 64);
        B.rimg_rowd = D.alloc_zero<int>((size_t)nv);
    }
    B.col_partner = D.alloc_raw<int>((size_t)std::max<long long>(H.col_total, 1));     // (entries beyond col_cnt are never read)
    B.col_a1 = D.alloc_raw<double>((size_t)std::max<long long>(H.col_total, 1));
    hs.mark("allocations + uploads");
    LaunchPlan P = plan_launches(robots_, H, variant_, opt_, tiling_allowed_, D.n_cu);
    D.tile_launches.clear();
    for (auto& L : P.tile_launches) {
        D.tile_launches.emplace_back(std::move(L));
        D.tile_launches.back().list = D.upload(D.tile_launches.back().tile_ids);
    }
    const bool no_tiles = P.tiles.empty();
    B.tile_of = D.upload(P.tile_of);
    B.tile_lidx = D.upload(P.tile_lidx);
    B.col_code = D.alloc_raw<int>(no_tiles ? 1 : (size_t)std::max<long long>(H.col_total, 1));
    B.tile_xh = D.alloc_zero<int>(std::max<size_t>(1, P.tiles.size()) * VXH_TILE_XH);
    B.tile_xhn = D.alloc_zero<int>(std::max<size_t>(1, P.tiles.size()));
    B.n_tiles = (int)P.tiles.size();
    B.tiles = D.upload(P.tiles);
    B.tile_vox = D.upload(P.tile_vox);
    B.tile_bond = D.upload(P.tile_bond);
    B.tile_bcls = D.upload(P.tile_bcls);
    B.tile_bslot = D.upload(P.tile_bslot);
    B.nx = std::max(P.nx_total, 64);
    B.xslot = D.upload(P.xslot);
    B.xplanes = P.any_fluid_tiles ? 28 : 16;
    B.xch = D.alloc_zero<unsigned long long>(no_tiles ? 1 : (size_t)3 * B.xplanes * B.nx);
    B.n_tmv = P.n_tmv; B.n_tf = P.n_tf;       // fluid tiles: their parts of the drag mesh
    B.tile_mvert = D.upload(P.tile_mvert); B.tile_mv0 = D.upload(P.tile_mv0); B.tile_facet = D.upload(P.tile_facet);
    B.tile_ffirst = D.upload(P.tile_ffirst); B.tile_fcount = D.upload(P.tile_fcount);
    B.tile_mvox = D.upload(P.tile_mvox);
    B.tile_mv = D.alloc_zero<unsigned long long>(std::max<size_t>(1, P.tiles.size()) * 3 * VXH_TILE_MV_STRIDE);
    D.n_rest = P.n_rest; D.n_all = P.n_all;
    D.streamed_all = D.upload(P.streamed_all);
    D.streamed_rest = D.upload(P.streamed_rest);
    D.groups.clear();
    for (size_t gi = 0; gi < P.groups.size(); ++gi) {
        D.groups.emplace_back(std::move(P.groups[gi]));
        Device::Group& g = D.groups.back();
        g.list = D.upload(g.robots);
        if (g.order_use) {
            for (int k = 0; k < 2; ++k) g.order_bits[k] = D.alloc_zero<unsigned long long>((size_t)(g.count + 63) / 64 + 1);
            g.order_perm = (int*)D.alloc_zero<unsigned long long>((size_t)order_ws_words(g.count));
            // the ordering kernel once, here: its first launch loads its code, 0.4 ms that would otherwise fall into the first long call
            launch_dispatch_order(order_ws_cost(g.order_perm, g.count), g.count, 0, g.order_perm, D.stream);
        }
        D.give_stream(g, gi);
    }
    D.reb_blocks = (int)P.reb_robot.size();
    D.reb_robot = D.upload(P.reb_robot);
    D.reb_i0 = D.upload(P.reb_i0);
#ifdef VXH_PHASE_TIMING
    B.prof = D.alloc_zero<unsigned long long>(VXH_PROF_WORDS);
#endif
    B.small_angle_w = std::cos(VXH_SMALL_ANGLE_RAD * 0.5);                    // Vec3D.h:55-59
    B.smallish_angle_w = std::cos(VXH_HYST * VXH_SMALL_ANGLE_RAD * 0.5);
    B.slthresh_acos2sqrt = 1.0 - 0.9988 * 0.9988;
    HIP_OK(hipStreamSynchronize(D.stream));      // every upload has left the host tables
    D.verify_uploads("at the end of prepare()");
    // what outlives the call: the rest of the host tables (hundreds of megabytes for a large population) ends here
    D.h_robot = std::move(H.robot);
    D.vox_begin = std::move(H.vox_begin); D.surf_begin = std::move(H.surf_begin); D.total_surf = ns;
    D.trace_begin = std::move(H.trace_begin); D.trace_cap = std::move(H.trace_cap); D.total_trace = H.total_trace;
    D.vol_begin = std::move(H.vol_begin); D.total_vol = H.total_vol; D.total_xtrace = H.total_xtrace;
    for (int k = 0; k < 2; ++k) { D.xt_begin[k] = std::move(H.xt_begin[k]); D.xt_cap[k] = std::move(H.xt_cap[k]); }
    D.max_planned = H.max_planned; D.max_nvox = H.max_nvox;
    D.robot_tiled = std::move(P.robot_tiled); D.robot_tiles = std::move(P.robot_tiles);
    hs.mark("kernel choice, tiling, launch groups");
    hs.print("prepare");
    forget_batch();
    prepared_ = true;
    counters_ = vxh_counters{};
}

void Engine::reset() { if (!robots_.empty()) prepare(); }

// (which kernel variant takes a robot -- fused_variant, wide_listed, resident_block -- is decided in batch.cpp; a Group carries the answer)
static void launch_group(const DBatch& B, int block, bool fluid, bool tabg, bool wide, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, int two_tiles = 0,
                         const unsigned long long* order_in = nullptr, unsigned long long* order_out = nullptr, bool cost = false)
{
    if (wide) { launch_wide_group(B, fluid, tabg, list, count, lds, s, cap, iters, two_tiles); return; }
    if (fluid) launch_fused_mesh(B, block, tabg, list, count, lds, s, cap, iters, order_in, order_out, cost);
    else launch_fused_land(B, block, tabg, list, count, lds, s, cap, iters, order_in, order_out, cost);
}

// A call in two halves: advance_launch enqueues every kernel of the call and returns; advance_finish waits for the device, reads
// the control blocks back and does the accounting.  advance() = one after the other; a handle that pipelines a generation over
// several engines of one device (EngineSet::run) launches them all before it waits for the first.
void Engine::advance(long long max_rounds)
{
    const long long before = rounds_done_;
    try {
        launch_and_finish(max_rounds);
    } catch (const TileTimeout& e) {
        // The tiles of a robot are co-resident workgroups that wait for each other: a second process on the GPU can keep some of them
        // off the chip until the bounded spins give up.  The robots' state of before the call is gone -- but the evaluation is a
        // deterministic function of the imported state, which the engine still holds: the batch is assembled again without the tiled
        // kernel (streaming kernels for what the resident one cannot take: slower, the same trajectories to 1e-12 voxel) and stepped
        // from the start up to where this call was to end -- a call in the middle of a run too (round 4; until then only a call that
        // started from the imported state was made again, and with several `voxelyze` processes on one GPU, the reference's own
        // launch pattern, this is the path that is hit).  The tiled kernel stays off for this engine.
        if (opt_.tiled == 0 || !tiling_allowed_) throw;
        std::fprintf(stderr, "vxhip: %s -- this batch is stepped again%s without the tiled kernel, which stays off for this engine\n", e.what(),
                     before != 0 ? " from its imported state" : "");
        opt_.tiled = 0;
        prepare();
        const long long huge = 0x7fffffffffffffffLL / 4;
        launch_and_finish(max_rounds >= huge - before ? huge : before + max_rounds);
    }
}

// a launch sequence that ended halfway (a refused kernel, a HIP error, a tile timeout): nothing of it may still be queued when the caller goes on
void Engine::launch_and_finish(long long max_rounds)
{
    try { advance_launch(max_rounds); advance_finish(); }
    catch (...) { quiesce(); throw; }
}

void Engine::quiesce()
{
    (void)hipSetDevice(device_id_);
    dev_->idle();
    dev_->pending.active = false;
}

void Engine::advance_launch(long long max_rounds)
{
    HIP_OK(hipSetDevice(device_id_));
    Device& D = *dev_;
    DBatch& B = D.B;
    const long long cap_all = 0x7fffffffffffffffLL;
    const long long remaining = std::max(0LL, D.max_planned - rounds_done_);
    const long long todo = std::min(max_rounds, remaining);
    const long long cap = (max_rounds >= remaining) ? cap_all : rounds_done_ + max_rounds;
    // robots that fit the resident kernel are stepped by their launch groups, the others (more than 1024 voxels, oversized
    // mesh) by the streaming kernels, side by side on their own streams; with the option fused = 0 everything streams
    const bool fused = opt_.fused && !D.groups.empty();
    const bool tiled = !D.tile_launches.empty();
    const bool streaming = fused ? D.n_rest > 0 : D.n_all > 0;
    B.streamed = fused ? D.streamed_rest : D.streamed_all;
    // per-robot step counts before, to attribute the work of this call
    if (D.pending.active) throw std::logic_error("a launched call has not been finished");
    std::vector<int>& steps_before = D.pending.steps_before;
    steps_before.assign(robots_.size(), 0);
    for (size_t r = 0; r < robots_.size(); ++r) steps_before[r] = host_.size() == robots_.size() ? host_[r].steps : 0;
    HostStages hs_l;
    HIP_OK(hipEventRecord(D.ev0, D.stream));
    hs_l.mark("first event");
    long long launches = 0;
    std::vector<long long>& group_launches = D.pending.group_launches;
    group_launches.assign(D.groups.size(), 0);
    // one launch group and nothing else (the usual population: robots of one size class): everything on the engine's own stream --
    // no event hand-offs between streams, which cost the command processor ~10-20 us each; a 20-step call is ~0.65 ms of kernel
    const bool single = fused && D.groups.size() == 1 && !tiled && !streaming;
    // (Tried in round 3 and taken out again: for short calls, the robots closest to their next broad-phase run dispatched first --
    // by displacement since the last one, from the previous call's control blocks -- so that the CUs that get them take fewer robots
    // afterwards.  The timed 20-step launch got 3 % shorter, 0.656 -> 0.634-0.650 ms; the host side of the call got 0.04-0.06 ms
    // longer in every variant tried -- list re-sorted and copied, partitioned and copied from pinned memory, read by the kernel from
    // mapped host memory -- which is more than the launch gained.  Polling the last event instead of sleeping on the stream: no gain.)
    if (fused) {
        const int iters = std::max(1, opt_.steps_per_launch);
        const bool prof_order = std::getenv("VXH_PROF_ORDER") != nullptr;      // (the spread under the list order too: dispatch_order = 0)
        for (auto& g : D.groups) {
            if (single) break;               // (its span is the call's: ev0 .. ev1; every event record is a packet the command processor works through)
            HIP_OK(hipStreamWaitEvent(g.stream, D.ev0, 0));
            HIP_OK(hipEventRecord(g.t0, g.stream));
        }
        for (long long done = 0; done < todo || done == 0; done += iters) {
            for (size_t k = 0; k < D.groups.size(); ++k) {
                auto& g = D.groups[k];
                // A short launch (what is left of the call, or the launch length itself): flagged robots first, flags for the next one.  A long
                // one: the robots by what they are expected to cost in it, longest first, from what the last long launch measured -- the
                // kernel instances that measure (COST), with k_dispatch_order in front (length 0: all keys equal, the list order).
                const long long len = std::min<long long>(iters, std::max<long long>(1, todo - done));
                const bool is_short = len <= VXH_ORDER_MAX_STEPS;
                const bool measure = g.order_use && !is_short && (opt_.dispatch_order != 0 || prof_order);
                const bool dyn = g.order_use && g.order_valid && is_short && opt_.dispatch_order != 0;
                hipStream_t st = single ? D.stream : g.stream;
                const unsigned long long* order_in = dyn ? g.order_bits[g.order_cur] : nullptr;
                if (measure) {
                    const bool by_cost = g.cost_valid && opt_.dispatch_order != 0;
                    launch_dispatch_order(order_ws_cost(g.order_perm, g.count), g.count, by_cost ? (int)len : 0, g.order_perm, st);
                    order_in = (const unsigned long long*)g.order_perm;
                    g.cost_valid = true; g.last_ordered = by_cost; g.last_len = len;
                }
                launch_group(B, g.block, g.fluid != 0, g.tabg != 0, g.wide != 0, g.list, g.count, g.lds, st, cap, iters, g.two_tiles, order_in,
                             g.order_use ? g.order_bits[g.order_cur ^ 1] : nullptr, measure);
                if (g.order_use) { g.order_cur ^= 1; g.order_valid = true; }      // (every launch leaves the flags for the next)
                ++launches; ++group_launches[k];
            }
        }
        if (!single) for (auto& g : D.groups) HIP_OK(hipEventRecord(g.t1, g.stream));
    }
    long long tile_launch_count = 0;
    if (tiled) {
        // every tiled launch on the one tile stream: the tiles of a robot wait for each other, so two such launches must never
        // compete for the CUs
        // ... nor with anything else: the launches are sized for an empty chip (`capacity` in prepare()), and the tiles of a robot that
        // are already placed spin -- holding their CUs -- until the missing ones arrive.  In a mixed batch the tiled launches therefore
        // run AFTER the launch groups of the resident robots, and the streaming kernels after them.
        const int iters = std::max(1, opt_.steps_per_launch);
        HIP_OK(hipStreamWaitEvent(D.tile_stream, D.ev0, 0));
        if (fused) for (auto& g : D.groups) HIP_OK(hipStreamWaitEvent(D.tile_stream, g.t1, 0));
        HIP_OK(hipEventRecord(D.tile_t0, D.tile_stream));
        for (long long done = 0; done < todo || done == 0; done += iters)
            for (const auto& L : D.tile_launches) {
                ++tile_gen_;
                launch_tile_group(B, L.tabg != 0, L.mesh, L.small != 0, L.list, L.count, L.lds, D.tile_stream, cap, iters, tile_gen_);
                ++launches; ++tile_launch_count;
            }
        HIP_OK(hipEventRecord(D.tile_t1, D.tile_stream));
    }
    if (streaming) {
        if (tiled) HIP_OK(hipStreamWaitEvent(D.stream, D.tile_t1, 0));
        auto round = [&](long long c) { launch_stream_round(B, D.any_fluid, D.reb_blocks, D.reb_robot, D.reb_i0, D.stream, c); };
        long long launched = 0;
        if (opt_.graph_steps > 1 && cap == cap_all && todo >= opt_.graph_steps) {
            if (!D.graph_exec || D.graph_rounds != opt_.graph_steps || D.graph_mask != B.streamed) {
                D.drop_graph();
                HIP_OK(hipStreamBeginCapture(D.stream, hipStreamCaptureModeThreadLocal));
                for (int k = 0; k < opt_.graph_steps; ++k) round(cap_all);
                HIP_OK(hipStreamEndCapture(D.stream, &D.graph));
                HIP_OK(hipGraphInstantiate(&D.graph_exec, D.graph, nullptr, nullptr, 0));
                D.graph_rounds = opt_.graph_steps;
                D.graph_mask = B.streamed;
            }
            while (todo - launched >= opt_.graph_steps) { HIP_OK(hipGraphLaunch(D.graph_exec, D.stream)); launched += opt_.graph_steps; }
        }
        for (; launched < todo; ++launched) round(cap);
        launch_stream_finish(B, D.stream, cap);
        launches += (D.any_fluid ? 5 : 3) * todo + 1;
    }
    if (fused && !single) for (auto& g : D.groups) HIP_OK(hipStreamWaitEvent(D.stream, g.t1, 0));
    if (tiled) HIP_OK(hipStreamWaitEvent(D.stream, D.tile_t1, 0));
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(D.ev1, D.stream));
    {   // the control blocks come back on the same stream, behind the kernels: one wait for both
        const size_t nr = robots_.size();
        if (D.h_rstate_cap < nr) throw std::logic_error("control-block mirror smaller than the batch");      // (sized by prepare())
        if (!(single && B.rstate_mirror))      // (one launch group and nothing else: its kernel has written the mirror itself)
            HIP_OK(hipMemcpyAsync(D.h_rstate, B.rstate, sizeof(DRobotState) * nr, hipMemcpyDeviceToHost, D.stream));
    }
    hs_l.mark("kernels + last event queued");
    hs_l.print("advance_launch");
    D.pending.active = true; D.pending.todo = todo; D.pending.launches = launches; D.pending.tile_launch_count = tile_launch_count;
    D.pending.fused = fused; D.pending.tiled = tiled; D.pending.streaming = streaming; D.pending.single = single;
}

void Engine::advance_finish()
{
    HIP_OK(hipSetDevice(device_id_));
    Device& D = *dev_;
    if (!D.pending.active) return;
    Device::Pending& P = D.pending;
    P.active = false;
    HostStages hs;
    HIP_OK(hipStreamSynchronize(D.stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
    counters_.kernel_seconds += ms * 1e-3;
    counters_.launches += P.launches;
    rounds_done_ += P.todo;
    state_downloaded_ = reduced_downloaded_ = false;
    hs.mark("wait for the GPU");
    download_control(true);
    hs.mark("control blocks back");
    if (P.fused && std::getenv("VXH_PROF_ORDER")) D.report_dispatch_cost();
    // dominant kernel of this call (batch.cpp decides which unit; here: the pair of events that timed it)
    std::vector<int>& steps = P.steps_before;                  // (from here on: the steps this call took)
    for (size_t r = 0; r < robots_.size(); ++r) steps[r] = host_[r].steps - steps[r];
    std::vector<const GroupPlan*> groups;
    for (const Device::Group& g : D.groups) groups.push_back(&g);
    const DominantKernel dom = dominant_kernel(robots_, steps, groups, D.robot_tiled, P.fused, P.tiled, P.streaming, D.n_rest, P.todo, P.group_launches, P.tile_launch_count);
    float cms = ms;
    if (dom.unit == DominantKernel::TILES) HIP_OK(hipEventElapsedTime(&cms, D.tile_t0, D.tile_t1));
    else if (dom.unit == DominantKernel::GROUP && !P.single) HIP_OK(hipEventElapsedTime(&cms, D.groups[dom.group].t0, D.groups[dom.group].t1));
    counters_.dominant_block = dom.block; counters_.dominant_robots = dom.robots;
    counters_.dominant_launches = dom.launches; counters_.dominant_seconds = cms * 1e-3;
    counters_.dominant_alg_bytes = dom.alg_bytes; counters_.dominant_voxel_steps = dom.voxel_steps;
    hs.mark("accounting");
    hs.print("advance_finish");
}

void Engine::run() { step(0x7fffffffffffffffLL / 4); }

void Engine::run_launch()
{
    if (robots_.empty()) return;
    if (!prepared_) prepare();
    advance_launch(0x7fffffffffffffffLL / 4);
}
void Engine::run_finish() { if (!robots_.empty()) advance_finish(); }

void Engine::step(long long n)
{
    auto t0 = std::chrono::steady_clock::now();
    if (robots_.empty() || n <= 0) return;
    if (!prepared_) prepare();
    advance(n);
    counters_.run_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// per-robot control blocks (a few hundred bytes each): status, step counts, IniCM -> counters
void Engine::download_control(bool already_copied)
{
    Device& D = *dev_;
    const int nr = (int)robots_.size();
    std::vector<DRobotState> own;
    const DRobotState* rstate = D.h_rstate;          // (already_copied: advance_launch queued the copy into the pinned mirror, advance_finish waited for it)
    if (!already_copied || !D.h_rstate) {
        own.resize(nr);
        HIP_OK(hipMemcpy(own.data(), D.B.rstate, sizeof(DRobotState) * nr, hipMemcpyDeviceToHost));
        rstate = own.data();
    }
    if ((int)host_.size() != nr) host_.assign(nr, HostState());
    double vs = 0, bs = 0, ab = 0; long long mx = 0;
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots_[r];
        HostState& H = host_[r];
        const DRobotState& S = rstate[r];
        H.cur_time = S.cur_time; H.steps = S.steps; H.status = S.status; H.cm_init = S.cm_init; H.rebuilds = S.rebuilds;
        H.eol_post_y = S.eol_post_y;
        H.cm_trace.assign((size_t)4 * std::min(S.ntrace, D.trace_cap[r]), 0.0);      // (filled by download())
        const bool norm_vol = variant_ == 0 && M.vxa.norm_dist_by_vol && D.trace_cap[r] > 0;      // (RF_NORM_VOL, batch.cpp)
        H.vol_trace.assign(norm_vol ? H.cm_trace.size() / 4 : 0, 0.0);
        for (int k = 0; k < 2; ++k) H.xtrace[k].assign((size_t)5 * std::min(S.nxtrace[k], D.xt_cap[k][r]), 0.0);
        for (int k = 0; k < 3; ++k) H.ini_cm[k] = S.ini_cm[k];
        if (S.col_overflow) H.status = VXH_ROBOT_COL_OVERFLOW;
        if (S.status == 5 || (r == 0 && inject_tile_timeout_ > 0 && !D.tile_launches.empty() && --inject_tile_timeout_ == 0)) {
            throw TileTimeout("HIP: the tiles of robot " + std::to_string(r) + " timed out waiting for each other (is another process "
                              "using this GPU? set the engine option tiled = 0 then)");
        }
        vs += (double)M.nvox * S.steps; bs += (double)M.nbond * S.steps; ab += (224.0 * M.nvox + 144.0 * M.nbond) * S.steps;
        mx = std::max(mx, (long long)S.steps);
    }
    counters_.voxel_steps = vs; counters_.bond_steps = bs; counters_.algorithmic_bytes = ab; counters_.max_steps = mx;
    control_downloaded_ = true;
}

// full voxel state (lazy: only when results or trajectories are requested)
void Engine::download()
{
    HIP_OK(hipSetDevice(device_id_));
    Device& D = *dev_;
    const DBatch& B = D.B;
    const int nr = (int)robots_.size(), nv = B.nv;
    if (!control_downloaded_) download_control();
    std::vector<double> planes((size_t)18 * nv);
    HIP_OK(hipMemcpy(planes.data(), B.vs, sizeof(double) * planes.size(), hipMemcpyDeviceToHost));
    auto plane = [&](int comp) { return planes.data() + (size_t)comp * nv; };
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots_[r];
        HostState& H = host_[r];
        const int n = M.nvox, base = D.vox_begin[r], b = H.steps & 1;
        H.pos.resize((size_t)3 * n); H.quat.resize((size_t)4 * n); H.scale.resize(n); H.lin_mom.resize((size_t)3 * n); H.ang_mom.resize((size_t)3 * n);
        for (int v = 0; v < n; ++v) {
            for (int k = 0; k < 3; ++k) { H.pos[3 * v + k] = plane(4 * b + k)[base + v]; H.lin_mom[3 * v + k] = plane(12 + k)[base + v]; H.ang_mom[3 * v + k] = plane(15 + k)[base + v]; }
            for (int k = 0; k < 4; ++k) H.quat[4 * v + k] = plane(8 + k)[base + v];
            H.scale[v] = plane(4 * b + 3)[base + v];
        }
    }
    // land_water robots: directional strains of the last step (RobotVolumeEnd)
    bool any_mesh = false;
    for (int r = 0; r < nr; ++r) any_mesh = any_mesh || robots_[r].nmv > 0;
    if (any_mesh) {
        std::vector<double> st((size_t)6 * nv);
        HIP_OK(hipMemcpy(st.data(), B.strain, sizeof(double) * st.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < nr; ++r) {
            const RobotModel& M = robots_[r];
            if (M.nmv == 0) continue;
            HostState& H = host_[r];
            H.strain.resize((size_t)6 * M.nvox);
            for (int v = 0; v < M.nvox; ++v)
                for (int k = 0; k < 6; ++k) H.strain[(size_t)6 * v + k] = st[(size_t)k * nv + D.vox_begin[r] + v];
        }
    } else {
        for (int r = 0; r < nr; ++r) host_[r].strain.clear();
    }
    state_downloaded_ = true;
}

const std::vector<double>& Engine::trace_of(int robot)
{
    if (!prepared_) throw std::logic_error("trace requested before vxh_run/vxh_step");
    if (!reduced_downloaded_) download_reduced();
    return host_[robot].cm_trace;
}

int Engine::cm_trace(int robot, double* out4n, int capacity)
{
    const std::vector<double>& t = trace_of(robot);
    const int n = (int)(t.size() / 4);
    for (int k = 0; k < std::min(n, capacity) * 4; ++k) out4n[k] = t[k];
    return n;
}

const HostState& Engine::traces_of(int robot)
{
    trace_of(robot);
    return host_[robot];
}

int Engine::cm_trace_of(int robot, int which, double* out4n, int capacity)
{
    if (which == VXH_TRACE_LIFE) return cm_trace(robot, out4n, capacity);
    if (which != VXH_TRACE_AFTERLIFE && which != VXH_TRACE_FROZEN) throw std::invalid_argument("which: 0 life, 1 after-life, 2 frozen");
    const std::vector<double>& t = traces_of(robot).xtrace[which - 1];
    const int n = (int)(t.size() / 5);
    for (int i = 0; i < std::min(n, capacity); ++i)
        for (int k = 0; k < 4; ++k) out4n[4 * i + k] = t[(size_t)5 * i + k];
    return n;
}

int Engine::volume_trace(int robot, int which, double* out2n, int capacity)
{
    if (which < VXH_TRACE_LIFE || which > VXH_TRACE_FROZEN) throw std::invalid_argument("which: 0 life, 1 after-life, 2 frozen");
    const HostState& H = traces_of(robot);
    if (which == VXH_TRACE_LIFE) {
        const int n = (int)H.vol_trace.size();
        for (int i = 0; i < std::min(n, capacity); ++i) { out2n[2 * i] = H.cm_trace[(size_t)4 * i]; out2n[2 * i + 1] = H.vol_trace[i]; }
        return n;
    }
    const std::vector<double>& t = H.xtrace[which - 1];
    const int n = (int)(t.size() / 5);
    for (int i = 0; i < std::min(n, capacity); ++i) { out2n[2 * i] = t[(size_t)5 * i]; out2n[2 * i + 1] = t[(size_t)5 * i + 4]; }
    return n;
}

std::vector<double> Engine::angle_excess(int robot, bool at_end)
{
    const RobotModel& M = robots_[robot];
    std::vector<double> out;
    if (!at_end) { mesh_angle_excess(M, nullptr, nullptr, nullptr, out); return out; }
    if (!prepared_) throw std::logic_error("angle excesses of the final state requested before vxh_run/vxh_step");
    if (!state_downloaded_) download();
    const HostState& H = host_[robot];
    if (H.steps == 0 || (int)H.strain.size() != 6 * M.nvox) mesh_angle_excess(M, nullptr, nullptr, nullptr, out);
    else mesh_angle_excess(M, H.pos.data(), H.quat.data(), H.strain.data(), out);
    return out;
}

void Engine::shape(int robot, bool at_end, MeshShape& out)
{
    const RobotModel& M = robots_[robot];
    if (!at_end) { mesh_shape(M, nullptr, nullptr, nullptr, out); return; }
    if (!prepared_) throw std::logic_error("the final mesh requested before vxh_run/vxh_step");
    if (!state_downloaded_) download();
    const HostState& H = host_[robot];
    if (H.steps == 0 || (int)H.strain.size() != 6 * M.nvox) mesh_shape(M, nullptr, nullptr, nullptr, out);
    else mesh_shape(M, H.pos.data(), H.quat.data(), H.strain.data(), out);
}

void Engine::bond_modes(long long* large_angle, long long* total)
{
    if (!prepared_) throw std::logic_error("bond modes requested before vxh_run/vxh_step");
    HIP_OK(hipSetDevice(device_id_));
    const int nv = dev_->B.nv;
    std::vector<unsigned char> flags((size_t)3 * nv);
    HIP_OK(hipMemcpy(flags.data(), dev_->B.small_angle, flags.size(), hipMemcpyDeviceToHost));
    long long l = 0, t = 0;
    for (size_t r = 0; r < robots_.size(); ++r) {
        const RobotModel& M = robots_[r];
        for (int v = 0; v < M.nvox; ++v)
            for (int a = 0; a < 3; ++a)
                if (M.bond_class[(size_t)v * 3 + a] >= 0) { ++t; if (!(flags[(size_t)a * nv + dev_->vox_begin[r] + v] & 1)) ++l; }
    }
    *large_angle = l; *total = t;
}

// What the results need of the final state, reduced on the device (k_results: 72 bytes per robot instead of 144 per voxel), and the
// centre-of-mass traces
void Engine::download_reduced()
{
    HIP_OK(hipSetDevice(device_id_));
    Device& D = *dev_;
    const int nr = (int)robots_.size();
    if (!control_downloaded_) download_control();
    if (nr > 0) {
        if (!D.results) D.results = D.alloc_zero<DResult>(nr);
        launch_results(D.B, nr, D.results, D.stream);
        HIP_OK(hipGetLastError());
        std::vector<DResult> h(nr);
        HIP_OK(hipMemcpyAsync(h.data(), D.results, sizeof(DResult) * nr, hipMemcpyDeviceToHost, D.stream));
        HIP_OK(hipStreamSynchronize(D.stream));
        for (int r = 0; r < nr; ++r) {
            HostState& H = host_[r];
            H.reduced = true;
            for (int k = 0; k < 3; ++k) H.red_cm[k] = h[r].cm[k];
            H.d2max = h[r].d2max; H.d2min = h[r].d2min; H.ymax = h[r].ymax; H.ymin = h[r].ymin; H.touching = h[r].touching; H.feet = h[r].feet;
        }
    }
    if (D.total_trace > 0) {
        std::vector<double> tr((size_t)D.total_trace * 4);
        HIP_OK(hipMemcpy(tr.data(), D.B.trace, sizeof(double) * tr.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < nr; ++r)
            for (size_t k = 0; k < host_[r].cm_trace.size(); ++k) host_[r].cm_trace[k] = tr[(size_t)D.trace_begin[r] * 4 + k];
    }
    if (D.total_vol > 0) {                 // robots with <NormDistByVol>: the volumes of those points, the after-life and frozen traces
        std::vector<double> tv((size_t)D.total_vol), tx((size_t)std::max(D.total_xtrace, 1) * 5);
        HIP_OK(hipMemcpy(tv.data(), D.B.trace_vol, sizeof(double) * tv.size(), hipMemcpyDeviceToHost));
        if (D.total_xtrace > 0) HIP_OK(hipMemcpy(tx.data(), D.B.xtrace, sizeof(double) * tx.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < nr; ++r) {
            HostState& H = host_[r];
            for (size_t k = 0; k < H.vol_trace.size(); ++k) H.vol_trace[k] = tv[(size_t)D.vol_begin[r] + k];
            for (int w = 0; w < 2; ++w)
                for (size_t k = 0; k < H.xtrace[w].size(); ++k) H.xtrace[w][k] = tx[(size_t)D.xt_begin[w][r] * 5 + k];
        }
    }
    reduced_downloaded_ = true;
}

void Engine::result(int robot, vxh_result* out)
{
    if (!prepared_) throw std::logic_error("results requested before vxh_run/vxh_step");
    // _voxcad: every tag from the device-side reductions; land_water: the RobotVolume tags need the surface mesh of the final state
    // (poses + strains of every voxel), evaluated on the host
    const bool need_state = variant_ == 1 || opt_.host_results;
    if (need_state && !state_downloaded_) download();
    if (!need_state && !reduced_downloaded_) download_reduced();
    if (variant_ == 0 && robots_[robot].vxa.norm_dist_by_vol && !reduced_downloaded_) download_reduced();   // (the traces the Norm tags are summed from)
    HostState& H = host_[robot];
    if (need_state) { const bool keep = H.reduced; H.reduced = false; compute_result(robots_[robot], H, out); H.reduced = keep; }
    else compute_result(robots_[robot], H, out);
}

void Engine::state14(int robot, double* out, int capacity)
{
    const RobotModel& M = robots_[robot];
    if (capacity < M.nvox) throw std::invalid_argument("state buffer too small");
    if (!prepared_) prepare();
    if (!state_downloaded_) download();
    const HostState& H = host_[robot];
    for (int v = 0; v < M.nvox; ++v) {
        const VoxClass& C = M.vox_classes[M.vox_class[v]];
        double* o = out + (size_t)14 * v;
        for (int k = 0; k < 3; ++k) o[k] = H.pos[3 * v + k];
        for (int k = 0; k < 4; ++k) o[3 + k] = H.quat[4 * v + k];
        o[7] = H.scale[v];
        for (int k = 0; k < 3; ++k) { o[8 + k] = H.lin_mom[3 * v + k] * C.mass_inv; o[11 + k] = H.ang_mom[3 * v + k] * C.inertia_inv; }
    }
}

}  // namespace vxh
