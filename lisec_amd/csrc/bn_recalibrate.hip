// BatchNormalization recalibration (LisecNet.recalibrate_batchnorm): the moving statistics of every BatchNormalization
// layer become statistics of the CURRENT variables over K sweeps -- what torch.optim.swa_utils.update_bn does with
// momentum=None -- without touching a finaliser.  Every finaliser in the tree updates a moving statistic as
//   m <- (float)((double)m*a + batch*(1 - a))
// so a training-mode forward over a ZEROED `state` (ParamStore.state, the one flat fp32 buffer of all moving statistics)
// leaves state[i] = fl32(batch_i * coef_i), coef_i = 1 - a of the finaliser that wrote it.  k_bn_recal_take, one launch
// behind each sweep's forward, divides that back out in fp64, adds the sweep to three fp64 planes of `acc` (S1 = sum of
// the means, S2 = sum of the variances, Sq = sum of the squared means) and zeroes the statistic for the next sweep;
// k_bn_recal_finish turns the sums into the new moving statistics, each rounded once to fp32:
//   LISEC_BN_STATS_MEAN    mean = S1/k, var = S2/k
//   LISEC_BN_STATS_POOLED  mean = S1/k, var = max(0, (S2/k + Sq/k) - mean*mean)
// The table (one record per layer: mean_off, var_off, C, coef) is a HOST array: it is validated and travels in the
// kernel arguments (at most LISEC_BN_RECAL_MAX_ENTRIES records, 2.3 KB), so nothing is uploaded and nothing is read from
// an address the host has not checked.  In the shape of csrc/weight_average.hip: no atomics, every channel owned by one
// thread, a grid-stride loop (blockIdx.x picks the record -- uniform, so the record is read with scalar loads --,
// blockIdx.y strides over its channels), the same bits from run to run.  A few thousand floats: launch latency is all
// there is to it.  The pad floats of `state` between the records are never read or written.
#include "bn.h"
#include "common.h"

// hipcc contracts a multiply into a following add or subtract by default (-ffp-contract=fast): Sq + m*m would become
// fma(m, m, Sq) and (S2/k + Sq/k) - mean*mean an fma too, one rounding short of the contract in include/lisec_hip.h
// (tests pin the bits against a numpy definition).  Contraction off: every operation below is an IEEE fp64 operation
// of its own, the divisions correctly rounded (no fast-math flag).
#pragma clang fp contract(off)

namespace lisec {
namespace {

// coef = 1 - momentum AS THE FINALISER COMPUTES IT, one constant per finaliser family.  They must match, to the bit:
//   k_bn_finalize (bn.hip)                          mmean*0.99 + mean*(1.0 - 0.99)                          -> kCoefConv
//   the in-kernel finaliser of a lisec_bn_sink (conv.h)   mm*0.99 + mean*(1.0 - 0.99)                       -> kCoefConv
//   the VFE finaliser (vfe.hip)     mmean*(double)kBnMomentum + mean*(1.0 - (double)kBnMomentum), 0.99f widened  -> kCoefVfe
// The two differ by 9.5e-7 relative, 16 x 2^-24: a layer given the other family's constant is that far off in every
// recalibrated statistic (tests/test_gpu_bn_recalibrate_net.py bounds a single sweep's mean by 3 x 2^-24).
constexpr double kCoefConv = 1.0 - 0.99;
constexpr double kCoefVfe = 1.0 - (double)kBnMomentum;

constexpr int kRecalThreads = 256;
constexpr int kRecalBlocksY = 8;        // channels of one record: at most 8 x 256 in flight, the rest by the stride

struct RecalTable {
    int n_entries;
    int total;                                       // N: the sum of C over the records
    int base[LISEC_BN_RECAL_MAX_ENTRIES];            // running channel index of a record's first channel
    lisec_bn_recal_entry e[LISEC_BN_RECAL_MAX_ENTRIES];
};

__global__ void __launch_bounds__(kRecalThreads)
k_bn_recal_take(float* __restrict__ state, RecalTable t, double* __restrict__ acc) {
    const lisec_bn_recal_entry& e = t.e[blockIdx.x];
    const int base = t.base[blockIdx.x];
    const double coef = e.coef;
    float* __restrict__ mean = state + e.mean_off;
    float* __restrict__ var = state + e.var_off;
    double* __restrict__ s1 = acc + base;
    double* __restrict__ s2 = acc + t.total + base;
    double* __restrict__ sq = acc + 2 * (long long)t.total + base;
    const int stride = gridDim.y * kRecalThreads;
    for (int c = blockIdx.y * kRecalThreads + threadIdx.x; c < e.C; c += stride) {
        const double m = (double)mean[c] / coef;
        const double v = (double)var[c] / coef;
        const double mm = m * m;
        s1[c] = s1[c] + m;
        s2[c] = s2[c] + v;
        sq[c] = sq[c] + mm;
        mean[c] = 0.f;
        var[c] = 0.f;
    }
}

__global__ void __launch_bounds__(kRecalThreads)
k_bn_recal_finish(float* __restrict__ state, RecalTable t, const double* __restrict__ acc, double k, int statistics) {
    const lisec_bn_recal_entry& e = t.e[blockIdx.x];
    const int base = t.base[blockIdx.x];
    float* __restrict__ mean = state + e.mean_off;
    float* __restrict__ var = state + e.var_off;
    const double* __restrict__ s1 = acc + base;
    const double* __restrict__ s2 = acc + t.total + base;
    const double* __restrict__ sq = acc + 2 * (long long)t.total + base;
    const int stride = gridDim.y * kRecalThreads;
    for (int c = blockIdx.y * kRecalThreads + threadIdx.x; c < e.C; c += stride) {
        const double m = s1[c] / k;
        double v = s2[c] / k;
        if (statistics == LISEC_BN_STATS_POOLED) {
            const double q = sq[c] / k;
            const double sum = v + q;
            const double mm = m * m;
            v = sum - mm;
            if (v < 0.0) v = 0.0;
        }
        mean[c] = (float)m;
        var[c] = (float)v;
    }
}

// the checks both entries share; fills *t.  The error text, or nullptr
const char* recal_table(const lisec_bn_recal_entry* table, int n_entries, RecalTable* t, int* max_c) {
    if (n_entries < 1 || n_entries > LISEC_BN_RECAL_MAX_ENTRIES) return "n_entries must lie in [1, LISEC_BN_RECAL_MAX_ENTRIES]";
    long long total = 0;
    *max_c = 0;
    for (int i = 0; i < n_entries; ++i) {
        const lisec_bn_recal_entry& e = table[i];
        if (e.C < 1) return "a record with C < 1";
        if (!(e.coef > 0.0 && e.coef < 1.0)) return "a record with coef outside (0, 1)";
        if (e.mean_off < 0 || e.var_off < 0 || e.mean_off % 4 || e.var_off % 4)
            return "a record whose offsets are negative or not multiples of 4 floats";
        t->base[i] = (int)total;
        t->e[i] = e;
        total += e.C;
        if (total > 0x7fffffffLL / 4) return "too many channels";
        if (e.C > *max_c) *max_c = e.C;
    }
    t->n_entries = n_entries;
    t->total = (int)total;
    return nullptr;
}

dim3 recal_grid(int n_entries, int max_c) {
    const int by = (max_c + kRecalThreads - 1) / kRecalThreads;
    return dim3((unsigned)n_entries, (unsigned)(by > kRecalBlocksY ? kRecalBlocksY : by));
}

}  // namespace
}  // namespace lisec

using namespace lisec;

extern "C" double lisec_bn_recalibrate_coef(int family) {
    return family == LISEC_BN_FINALIZER_CONV ? kCoefConv : family == LISEC_BN_FINALIZER_VFE ? kCoefVfe : 0.0;
}

extern "C" int lisec_bn_recalibrate_take(float* state, const lisec_bn_recal_entry* table, int n_entries, double* acc,
                                         lisec_stream_t stream_) {
    LISEC_CHECK_ARG(state && table && acc, "bn_recalibrate_take: NULL state, table or acc");
    LISEC_CHECK_ARG(reinterpret_cast<uintptr_t>(state) % 4 == 0 && reinterpret_cast<uintptr_t>(acc) % 8 == 0,
                    "bn_recalibrate_take: state must be 4-byte and acc 8-byte aligned");
    RecalTable t = {};
    int max_c = 0;
    const char* bad = recal_table(table, n_entries, &t, &max_c);
    LISEC_CHECK_ARG(!bad, "bn_recalibrate_take: %s (n_entries %d)", bad, n_entries);
    LISEC_LAUNCH(k_bn_recal_take, recal_grid(n_entries, max_c), dim3(kRecalThreads), 0, static_cast<hipStream_t>(stream_),
                 state, t, acc);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}

extern "C" int lisec_bn_recalibrate_finish(float* state, const lisec_bn_recal_entry* table, int n_entries, const double* acc,
                                           long long sweeps, int statistics, lisec_stream_t stream_) {
    LISEC_CHECK_ARG(state && table && acc, "bn_recalibrate_finish: NULL state, table or acc");
    LISEC_CHECK_ARG(reinterpret_cast<uintptr_t>(state) % 4 == 0 && reinterpret_cast<uintptr_t>(acc) % 8 == 0,
                    "bn_recalibrate_finish: state must be 4-byte and acc 8-byte aligned");
    LISEC_CHECK_ARG(sweeps >= 1, "bn_recalibrate_finish: sweeps = %lld must be >= 1", sweeps);
    LISEC_CHECK_ARG(statistics == LISEC_BN_STATS_MEAN || statistics == LISEC_BN_STATS_POOLED,
                    "bn_recalibrate_finish: unknown statistics %d", statistics);
    RecalTable t = {};
    int max_c = 0;
    const char* bad = recal_table(table, n_entries, &t, &max_c);
    LISEC_CHECK_ARG(!bad, "bn_recalibrate_finish: %s (n_entries %d)", bad, n_entries);
    LISEC_LAUNCH(k_bn_recal_finish, recal_grid(n_entries, max_c), dim3(kRecalThreads), 0, static_cast<hipStream_t>(stream_),
                 state, t, acc, (double)sweeps, statistics);
    LISEC_LAUNCH_CHECK();
    return LISEC_OK;
}
