// Error reporting, version and the optional per-kernel-class event profiler of the C ABI.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "common.hpp"
#include "tn_plan.hpp"
#include "../../include/clip_event_hip.h"

static thread_local char g_err[512] = "";

void ce_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* ce_last_error(void) { return g_err; }
extern "C" int ce_version(void) { return 1; }

// ---- fp16 residual / gradient stream: saturation telemetry (include/clip_event_hip.h, ce_stream16_set_counters) ----
// One process drives one GPU, so a single registered buffer serves every launch of the process.
static unsigned int* g_sat_counters = nullptr;
extern "C" int ce_stream16_set_counters(unsigned int* device_counters) {
    g_sat_counters = device_counters;
    return 0;
}
unsigned int* ce_sat_counters() { return g_sat_counters; }

// ---- the process's weight-gradient GEMM switches: the environment, read once (the TN launcher and the profiler's names) ----
const TNKnobs& tn_process_knobs() {
    static const TNKnobs knobs = tn_knobs_from_env();
    return knobs;
}

// ---- profiler: HIP events recorded on the launch stream around every launch of a class ----
namespace {
struct Rec { int cls; double flops, bytes; hipEvent_t e0, e1; };
std::mutex g_mu;
bool g_on = false;
std::vector<Rec> g_recs;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_pool;
const char* kEpi[9] = {"BF16", "F32", "BIAS_BF16", "BIAS_F32", "BIAS_RESID_F32", "BIAS_GELU", "GELUGRAD_BF16", "BIAS_RESID_F16", "BIAS_QGELU_BF16"};
const char* kFam[CE_PROF_NT_FAMILIES] = {"gemm_nt_kernel<%d>", "gemm_nt256_kernel<%d,*,2>", "gemm_nt256_kernel<%d,*,4>",
                                         "gemm_nt32_kernel<%d>", "gemm_nt8_kernel<%d,*,*>", "gemm_nt160lw_kernel<%d,*>",
                                         "gemm_nt160p_kernel<%d,*>", "gemm_nt_skinny_kernel<%d>"};
const char* kRest[CE_PROF_GEMM_NT_QGELU - CE_PROF_GEMM_TN] = {"gemm_tn3_kernel", "attn_fwd", "attn_bwd", "ln_fwd", "ln_bwd",
                                                       "colsum_bf16", "other", "gemm_tn2_kernel"};
thread_local char g_name[96];
}  // namespace

int ce_prof_begin(int cls, double flops, double bytes, hipStream_t s) {
    if (!g_on) return -1;
    std::lock_guard<std::mutex> lk(g_mu);
    Rec r;
    r.cls = cls; r.flops = flops; r.bytes = bytes;
    if (!g_pool.empty()) {
        r.e0 = g_pool.back().first; r.e1 = g_pool.back().second; g_pool.pop_back();
    } else {
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
    }
    hipEventRecord(r.e0, s);
    g_recs.push_back(r);
    return (int)g_recs.size() - 1;
}

void ce_prof_end(int idx, hipStream_t s) {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_mu);
    if (idx < (int)g_recs.size()) hipEventRecord(g_recs[idx].e1, s);
}

extern "C" void ce_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_on = on != 0;
}

extern "C" const char* ce_profile_class_name(int cls) {
    if (cls < 0 || cls >= CE_PROF_NCLASS) return "?";
    if (cls == CE_PROF_GEMM_TN) {      // the rocprofv3 row of whichever 256x256 form the launcher uses (csrc/gemm.hip)
        return tn_process_knobs().loader_waves ? "gemm_tn3lw_kernel" : "gemm_tn3_kernel";
    }
    if (cls >= CE_PROF_GEMM_TN && cls < CE_PROF_GEMM_NT_QGELU) return kRest[cls - CE_PROF_GEMM_TN];
    const int epi = cls >= CE_PROF_GEMM_NT_QGELU ? CE_EPI_BIAS_QGELU_BF16 : cls / CE_PROF_NT_FAMILIES;
    char fam[64];
    snprintf(fam, sizeof(fam), kFam[cls % CE_PROF_NT_FAMILIES], epi);
    snprintf(g_name, sizeof(g_name), "%s %s", fam, kEpi[epi]);       // e.g. "gemm_nt256_kernel<0,*,2> BF16"
    return g_name;
}

extern "C" int ce_profile_num_classes(void) { return CE_PROF_NCLASS; }

void ce_prof_retag(int idx, int cls) {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lk(g_mu);
    if (idx < (int)g_recs.size()) g_recs[idx].cls = cls;
}

extern "C" int ce_profile_collect(double* out, int max_classes) {
    std::lock_guard<std::mutex> lk(g_mu);
    const int n = max_classes < CE_PROF_NCLASS ? max_classes : CE_PROF_NCLASS;
    for (int i = 0; i < n * 4; ++i) out[i] = 0.0;
    for (auto& r : g_recs) {
        hipEventSynchronize(r.e1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        if (r.cls >= 0 && r.cls < n) {
            out[r.cls * 4 + 0] += 1.0;
            out[r.cls * 4 + 1] += ms;
            out[r.cls * 4 + 2] += r.flops;
            out[r.cls * 4 + 3] += r.bytes;
        }
        g_pool.emplace_back(r.e0, r.e1);
    }
    g_recs.clear();
    return n;
}
