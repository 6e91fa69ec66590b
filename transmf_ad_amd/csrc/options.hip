// options.hip — the library's process options: tmf_set_option, the TMF_* environment and the per-call algorithm word
// (tmf_snet_desc.flags with TMF_SNET_ALGO), one table row per option.  Host code only; include/tmf_hip.h lists the options.
//
// tmf_opt(o): for an option the per-call word carries, the calling entry's choice while a TmfAlgoScope holds one; else the value
// tmf_set_option gave; else the environment's (every variable is read once, on first use); else the default.  The set values are
// relaxed atomics: PyTorch runs backward on its own thread, which plans launches while the main thread may set an option.
#include "tmf_common.h"
#include <atomic>
#include <climits>

namespace {

constexpr int UNSET = INT_MIN;   // no tmf_set_option value (so "debug" INT_MIN reads as 0: the kernels test its low bits only)

int nonzero(int v) { return v != 0; }
int clamp02(int v) { return v <= 0 ? 0 : (v >= 2 ? 2 : 1); }
bool in02(int v) { return v >= 0 && v <= 2; }

struct Row {
    TmfOpt opt;
    const char* name;         // tmf_set_option name; nullptr: the environment only
    const char* env;          // environment variable; nullptr: tmf_set_option only
    int def;
    const char* accepts;      // tmf_set_option refuses what ok() does not take: "<name> must be <accepts>, got <value>"
    bool (*ok)(int);          // nullptr: any value
    int (*set)(int);          // tmf_set_option's value -> the option's (UNSET: back to the environment / default); nullptr: as given
    int (*from_env)(int);     // atoi of the variable -> the option's; nullptr: as given
    int call[3];              // the per-call word's bits that select values 1, 2, 3; none: not a per-call option
};

constexpr Row kRows[] = {
    {TMF_OPT_CONV_WINO, "conv_wino", "TMF_CONV_WINO", 3, "0, 1, 2 or 3", [](int v) { return v >= 0 && v <= 3; }, nullptr,
     [](int v) { return v >= 0 && v <= 2 ? v : 3; }, {TMF_SNET_ALGO_WINO(1), TMF_SNET_ALGO_WINO(2), TMF_SNET_ALGO_WINO(3)}},
    {TMF_OPT_WINO_P, "wino_p", "TMF_WINO_P", 1, nullptr, nullptr, nonzero, nonzero, {TMF_SNET_ALGO_WINO_P}},
    {TMF_OPT_WINO_X, "wino_x", "TMF_WINO_X", 1, nullptr, nullptr, nonzero, nonzero, {TMF_SNET_ALGO_WINO_X}},
    {TMF_OPT_C1_GRAM, "c1_gram", "TMF_C1_GRAM", 1, nullptr, nullptr, clamp02, clamp02,
     {TMF_SNET_ALGO_C1_GRAM, TMF_SNET_ALGO_C1_GRAM | TMF_SNET_ALGO_C1_GRAM_BF16}},
    {TMF_OPT_C1_SPLIT, "c1_split", "TMF_C1_SPLIT", 1, nullptr, nullptr, nonzero, nonzero, {TMF_SNET_ALGO_C1_SPLIT}},
    {TMF_OPT_POOL_RECOMPUTE, "pool_recompute", "TMF_POOL_RECOMPUTE", 0, "0, 1, 2 or 3", [](int v) { return v >= 0 && v <= 3; }, nullptr,
     [](int v) { return v >= 0 && v <= 3 ? v : 0; },
     {TMF_SNET_ALGO_POOL_REC_C1 | TMF_SNET_ALGO_POOL_REC_BN, TMF_SNET_ALGO_POOL_REC_C1, TMF_SNET_ALGO_POOL_REC_BN}},
    {TMF_OPT_WINO_CUS, "wino_cus", "TMF_WINO_CUS", 0, ">= 0", [](int v) { return v >= 0; }, [](int v) { return v ? v : UNSET; },
     nullptr, {}},
    {TMF_OPT_CONV_RT, "conv_rt", "TMF_CONV_RT", 0, "0, 1 or 2", in02, nullptr, [](int v) { return v == 1 || v == 2 ? v : 0; }, {}},
    {TMF_OPT_CONV_WAVES, "conv_waves", "TMF_CONV_WAVES", 16, "2, 4, 8 or 16", [](int v) { return v == 2 || v == 4 || v == 8 || v == 16; },
     nullptr, [](int v) { return v == 2 || v == 4 || v == 8 ? v : 16; }, {}},
    {TMF_OPT_BF16_V2, "bf16_v2", "TMF_BF_V2", 1, "0, 1 or 2", in02, nullptr, [](int v) { return v == 0 || v == 2 ? v : 1; }, {}},
    {TMF_OPT_BF16_DMA, "bf16_dma", nullptr, 1, "0 or 1", [](int v) { return v == 0 || v == 1; }, nullptr, nullptr, {}},
    {TMF_OPT_WGRAD_TR, "wgrad_tr", nullptr, 1, "0, 1 or 2", in02, nullptr, nullptr, {}},
    {TMF_OPT_DEBUG, "debug", nullptr, 0, nullptr, nullptr, nullptr, nullptr, {}},
    {TMF_OPT_WINO_EVEN, nullptr, "TMF_WINO_EVEN", 1, nullptr, nullptr, nullptr, nonzero, {}},
    {TMF_OPT_WINOX_SWAP, nullptr, "TMF_WINOX_SWAP", 1, nullptr, nullptr, nullptr, nonzero, {}},
    {TMF_OPT_BF_NT2, nullptr, "TMF_BF_NT2", 1, nullptr, nullptr, nullptr, nonzero, {}},
    {TMF_OPT_CONV_AUTO, nullptr, "TMF_CONV_AUTO", 1, nullptr, nullptr, nullptr, nonzero, {}},
    {TMF_OPT_C1_BLOCKS, nullptr, "TMF_C1_BLOCKS", 1024, nullptr, nullptr, nullptr, [](int v) { return v < 64 ? 1024 : v; }, {}},
    {TMF_OPT_C1_FWD_MULT, nullptr, "TMF_C1_FWD_MULT", 4, nullptr, nullptr, nullptr, nullptr, {}},
};
constexpr bool rows_in_order() {
    for (int o = 0; o < TMF_OPT_COUNT; ++o)
        if (kRows[o].opt != o) return false;
    return sizeof kRows / sizeof kRows[0] == TMF_OPT_COUNT;
}
static_assert(rows_in_order(), "kRows: one row per TmfOpt, in the enum's order");

struct Values {
    int env[TMF_OPT_COUNT];                 // the environment's value, the default where the variable is not set
    std::atomic<int> set[TMF_OPT_COUNT];    // tmf_set_option's value or UNSET
    Values() {
        for (const Row& r : kRows) {
            const char* e = r.env ? getenv(r.env) : nullptr;
            env[r.opt] = e == nullptr ? r.def : (r.from_env ? r.from_env(atoi(e)) : atoi(e));
            set[r.opt].store(UNSET, std::memory_order_relaxed);
        }
    }
};
Values& values() {
    static Values v;      // (thread-safe initialisation: the environment is read once)
    return v;
}

thread_local int t_algo = 0;        // the per-call word a TmfAlgoScope holds on this thread, or 0

}  // namespace

TmfAlgoScope::TmfAlgoScope(int flags) : prev(t_algo) { if (flags & TMF_SNET_ALGO) t_algo = flags; }
TmfAlgoScope::~TmfAlgoScope() { t_algo = prev; }

int tmf_opt(TmfOpt o) {
    const Row& r = kRows[o];
    if (r.call[0]) {
        if (const int f = t_algo) {
            const int bits = f & (r.call[0] | r.call[1] | r.call[2]);
            for (int i = 0; i < 3; ++i)
                if (r.call[i] && bits == r.call[i]) return i + 1;
            return 0;
        }
    }
    Values& v = values();
    const int s = v.set[o].load(std::memory_order_relaxed);
    return s != UNSET ? s : v.env[o];
}

extern "C" int tmf_set_option(const char* name, int value) {
    TMF_REQUIRE_PTR(name);
    for (const Row& r : kRows) {
        if (r.name == nullptr || strcmp(name, r.name) != 0) continue;
        TMF_REQUIRE(r.ok == nullptr || r.ok(value), TMF_E_ARG, "tmf_set_option: %s must be %s, got %d", r.name, r.accepts, value);
        values().set[r.opt].store(r.set ? r.set(value) : value, std::memory_order_relaxed);
        return TMF_OK;
    }
    tmf_set_error("tmf_set_option: unknown option '%s'", name);
    return TMF_E_ARG;
}

extern "C" int tmf_snet_algo_flags(void) {
    int flags = TMF_SNET_ALGO;
    for (const Row& r : kRows)
        if (const int v = r.call[0] ? tmf_opt(r.opt) : 0) flags |= r.call[v - 1];
    return flags;
}

extern "C" int tmf_conv_wino_mode(void) { return tmf_opt(TMF_OPT_CONV_WINO); }
extern "C" int tmf_wino_p_mode(void) { return tmf_opt(TMF_OPT_WINO_P); }
extern "C" int tmf_wino_x_mode(void) { return tmf_opt(TMF_OPT_WINO_X); }
extern "C" int tmf_c1_split_mode(void) { return tmf_opt(TMF_OPT_C1_SPLIT); }
