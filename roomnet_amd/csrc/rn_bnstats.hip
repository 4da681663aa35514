// Batch-statistics BatchNorm (RN_FLAG_BATCH_STATS): what tf.layers.batch_normalization(training=True) computes in the forward pass
// of the reference's default model (compute_bn_mean_var=True; network.py:193, :202, :217).  Float32 per-node handles only: at each
// of the 16 BN nodes the forward pass launches
//   moments   per-channel mean and M2 = sum (x - mean)^2 of the node's input over n * h * w, one pass over the tensor
//   finalise  merges the workgroups' partials and writes the node's (mean, inv = rsqrt(var + eps) * gamma) table on the device
// and then the SAME bn_f32_kernel as an inference handle, reading that table (beta is the checkpoint's).  The three normalised
// dense blocks (moments over the batch axis only) run as dense -> ReLU6, then moments + BN in one workgroup; the last block, the
// softmax and the argmax are head_kernel's.
//
// Arithmetic of the moments.  n * h * w reaches 1.2e7 (256 x 220 x 220): a float32 running sum loses 3 digits there, and
// E[x^2] - E[x]^2 cancels.  Every thread runs Welford's recurrence in float32 over the <= few hundred float4 it reads (one
// reciprocal per float4: a thread's four channels share the count); from there on everything is a merge of (n, mean, M2)
// triples by Chan's rule in float64:  n = na + nb, d = mb - ma, mean = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n  -- pairwise
// across a wavefront (xor shuffles) and across the workgroup's four wavefronts (LDS), and in its k-way form
//   mean = sum n_b mean_b / sum n_b,   M2 = sum M2_b + sum n_b (mean_b - mean)^2
// over the workgroups' partials in the finalise launch.  Grid, thread -> element assignment and merge order are fixed by the
// tensor's shape alone and there is no atomic: two calls on one input give the same bits.
#include "rn_internal.h"
#include "rn_fused.h"

#include <algorithm>
#include <new>

namespace {

constexpr int MOM_THREADS = 256;
constexpr int MOM_MAX_BLOCKS = 2048;      // 8 workgroups per CU on 256 CUs; longer tensors are grid-strided
constexpr int MOM_MIN_F4_PER_THREAD = 8;  // (short tensors: fewer workgroups rather than threads with one element each)
constexpr int MAX_BN_CHANNELS = 128;

struct Part {                              // one (workgroup, channel) partial
    double n, mean, m2;
};

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// Chan's rule: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb).  An empty side (n = 0, mean = 0, M2 = 0) is the neutral element.
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
    const double n = na + nb;
    const double f = n > 0 ? nb / n : 0.0;
    const double d = mb - ma;
    ma = ma + d * f;
    qa = qa + qb + d * d * na * f;
    na = n;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);      // (a + b == b + a: every lane ends with the same bits)
    return v;
}

// x: NHWC float32 seen as float4 [total4]; C / 4 consecutive float4 are one pixel.  256 and the grid stride are multiples of
// C / 4, so a thread meets the same four channels (4 (tid % (C / 4)) ..) in every float4 it reads; a wavefront's 64 lanes read
// 1 KiB contiguously per load, four loads in flight per thread.
template <int C>
__global__ __launch_bounds__(MOM_THREADS) void bn_moments_kernel(const float4* __restrict__ x, int64_t total4, Part* __restrict__ parts) {
    constexpr int G = C / 4;
    static_assert(C % 4 == 0 && G >= 2 && G <= 32 && (G & (G - 1)) == 0, "channel groups must divide a half wavefront");
    const int64_t stride = static_cast<int64_t>(gridDim.x) * MOM_THREADS;
    int64_t i = static_cast<int64_t>(blockIdx.x) * MOM_THREADS + threadIdx.x;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    const auto welford = [&](const float4& v) {
        ++k;
        const float r = __builtin_amdgcn_rcpf(static_cast<float>(k));
        const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = xs[j] - mean[j];
            mean[j] = fmaf(d, r, mean[j]);
            m2[j] = fmaf(d, xs[j] - mean[j], m2[j]);
        }
    };
    for (; i + 3 * stride < total4; i += 4 * stride) {
        const float4 v0 = x[i], v1 = x[i + stride], v2 = x[i + 2 * stride], v3 = x[i + 3 * stride];
        welford(v0);
        welford(v1);
        welford(v2);
        welford(v3);
    }
    for (; i < total4; i += stride) welford(x[i]);
    // lanes l, l + G, l + 2 G, ... of a wavefront hold the same channels: merge them pairwise
    double n = k, m[4], q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = mean[j];
        q[j] = m2[j];
    }
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) {
        const double nb = __shfl_xor(n, off);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double mb = __shfl_xor(m[j], off), qb = __shfl_xor(q[j], off);
            double nj = n;
            chan_merge(nj, m[j], q[j], nb, mb, qb);
        }
        n += nb;
    }
    __shared__ double sh[MOM_THREADS / 64][32][9];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < G) {
        sh[wave][lane][0] = n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sh[wave][lane][1 + j] = m[j];
            sh[wave][lane][5 + j] = q[j];
        }
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int g = threadIdx.x >> 2, j = threadIdx.x & 3;
        double na = sh[0][g][0], ma = sh[0][g][1 + j], qa = sh[0][g][5 + j];
        for (int w = 1; w < MOM_THREADS / 64; ++w) chan_merge(na, ma, qa, sh[w][g][0], sh[w][g][1 + j], sh[w][g][5 + j]);
        parts[static_cast<int64_t>(blockIdx.x) * C + threadIdx.x] = Part{na, ma, qa};
    }
}

// One wavefront per channel: k-way merge of the workgroups' partials, then the table bn_f32_kernel reads.  inv is formed from
// the float32 variance exactly as rn_create forms it from a checkpoint's moving_variance (rn_bn_inv): a handle created on these
// moments as moving statistics normalises with the same table.
__global__ __launch_bounds__(64) void bn_finalise_kernel(const Part* __restrict__ parts, int nparts, int C, const float* __restrict__ gamma,
                                                         float eps, float* __restrict__ mean_out, float* __restrict__ var_out,
                                                         float* __restrict__ inv_out, double* __restrict__ n_out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    double sn = 0, snm = 0;
    for (int b = lane; b < nparts; b += 64) {
        const Part p = parts[static_cast<int64_t>(b) * C + c];
        sn += p.n;
        snm = fma(p.n, p.mean, snm);
    }
    sn = wave_sum(sn);
    snm = wave_sum(snm);
    const double mean = snm / sn;
    double q = 0;
    for (int b = lane; b < nparts; b += 64) {
        const Part p = parts[static_cast<int64_t>(b) * C + c];
        const double d = p.mean - mean;
        q += p.m2 + p.n * d * d;
    }
    q = wave_sum(q);
    if (lane == 0) {
        const float var = static_cast<float>(q / sn);
        mean_out[c] = static_cast<float>(mean);
        var_out[c] = var;
        // sqrtf, not __fsqrt_rn: the intrinsic is the hardware's one-ulp square root here, sqrtf and the division are correctly
        // rounded, as the host's are in rn_bn_inv.  That rests on hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt: no
        // fast-math flag and no -fno-hip-fp32-correctly-rounded-divide-sqrt may reach build.sh
        // (tests/test_hip_bnstats_local.py's output check sees an inv one ulp off)
        inv_out[c] = __fmul_rn(__fdiv_rn(1.0f, sqrtf(__fadd_rn(var, eps))), gamma[c]);
        n_out[c] = sn;      // the count this channel's merge really saw (rn_bn_batch_stats reports it)
    }
}

// One dense block up to its ReLU6 (network.py:212-214), one workgroup per image: head_kernel's sums in head_kernel's order
// (a 64-thread workgroup: one fma chain over k per output; 1024 threads for a long flatten: k split over 1024 / nout
// partitions whose sums meet in LDS).  Writes the tap nodes dK.mm and dK.relu.
constexpr int DENSE_MAX_IN = 4096;
__global__ __launch_bounds__(1024) void dense_relu6_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                          int nin, int nout, float* __restrict__ mm, float* __restrict__ relu) {
    __shared__ float xin[DENSE_MAX_IN];
    __shared__ float part[1024];
    const int img = blockIdx.x, lane = threadIdx.x, nthr = blockDim.x;
    for (int i = lane; i < nin; i += nthr) xin[i] = in[static_cast<int64_t>(img) * nin + i];
    __syncthreads();
    const int parts = (nthr > 64 && nin > 64) ? nthr / nout : 1;
    if (parts > 1) {
        const int o = lane % nout, p = lane / nout;
        float v = 0.f;
        if (p < parts)
            for (int k = p; k < nin; k += parts) v = fmaf(xin[k], w[k * nout + o], v);
        part[lane] = v;
        __syncthreads();
    }
    if (lane < nout) {
        float v = 0.f;
        if (parts > 1) {
            for (int p = 0; p < parts; ++p) v += part[p * nout + lane];
        } else {
            for (int k = 0; k < nin; ++k) v = fmaf(xin[k], w[k * nout + lane], v);
        }
        if (bias) v = __fadd_rn(v, bias[lane]);
        mm[static_cast<int64_t>(img) * nout + lane] = v;
        relu[static_cast<int64_t>(img) * nout + lane] = relu6f(v);
    }
}

// BN of a dense block with the moments of the batch (network.py:217: rank 2, moments over axis 0): x is dK.relu [n, nout].  One
// workgroup for the whole batch; n values per channel are few: two passes in float64 (mean, then centred squares), one thread per
// channel, in image order.  y = x * inv + (beta - mean * inv), tf.nn.batch_normalization's form as head_kernel evaluates it.
// n = 1: variance 0, y = beta up to the rounding of x * inv.
__global__ __launch_bounds__(256) void dense_bn_batch_kernel(const float* __restrict__ x, int n, int nout, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ mean_out,
                                                             float* __restrict__ var_out, float* __restrict__ inv_out,
                                                             float* __restrict__ shift_out, double* __restrict__ n_out, float* __restrict__ y) {
    __shared__ float s_inv[64], s_shift[64];
    const int t = threadIdx.x;
    if (t < nout) {
        double s = 0;
        for (int i = 0; i < n; ++i) s += static_cast<double>(x[static_cast<int64_t>(i) * nout + t]);
        const double mean = s / n;
        double q = 0;
        for (int i = 0; i < n; ++i) {
            const double d = static_cast<double>(x[static_cast<int64_t>(i) * nout + t]) - mean;
            q = fma(d, d, q);
        }
        const float meanf = static_cast<float>(mean), var = static_cast<float>(q / n);
        const float inv = __fmul_rn(__fdiv_rn(1.0f, sqrtf(__fadd_rn(var, eps))), gamma[t]);      // (sqrtf: see bn_finalise_kernel)
        const float shift = __fsub_rn(beta[t], __fmul_rn(meanf, inv));
        mean_out[t] = meanf;
        var_out[t] = var;
        inv_out[t] = inv;
        shift_out[t] = shift;
        n_out[t] = n;
        s_inv[t] = inv;
        s_shift[t] = shift;
    }
    __syncthreads();
    for (int i = t; i < n * nout; i += 256) {
        const int c = i % nout;
        y[i] = __fadd_rn(__fmul_rn(x[i], s_inv[c]), s_shift[c]);
    }
}

// one BN of the graph, in the reference's variable order (batch_normalization, _1, ... _15)
struct BnSlot {
    int node = -1;              // its output node (sK.bn, sK.bn2, dK.bn)
    int c = 0;
    int64_t per_image = 1;      // h * w of the node: the moments are over last_n * per_image values
    float* gamma = nullptr;     // [c] device
    float* beta = nullptr;      // [c] device (dense BNs; the conv-side table keeps its own)
    float* mean = nullptr;      // [c] device: the last call's batch mean ...
    float* var = nullptr;       // ... and biased variance
    double* merged_n = nullptr; // [c] device: how many values the last call's merge saw per channel (the count rn_bn_batch_stats returns)
    float* inv = nullptr;       // the table entries the BN launch reads (conv side: BnDev.mean / .inv; dense: DensePlan.inv / .shift)
    float* shift = nullptr;
};

struct BnStatsPlan {
    std::vector<BnSlot> bns;
    std::vector<int> stage_bn, stage_bn2, dense_bn;     // index into bns (-1: none)
    Part* parts = nullptr;                               // [MOM_MAX_BLOCKS][MAX_BN_CHANNELS]
};

BnStatsPlan* plan_of(const rn_handle* h) { return static_cast<BnStatsPlan*>(h->bnstats); }

int moments_blocks(int64_t total4) {
    const int64_t want = (total4 + static_cast<int64_t>(MOM_THREADS) * MOM_MIN_F4_PER_THREAD - 1) / (static_cast<int64_t>(MOM_THREADS) * MOM_MIN_F4_PER_THREAD);
    return static_cast<int>(std::min<int64_t>(std::max<int64_t>(want, 1), MOM_MAX_BLOCKS));
}

template <int C>
void launch_moments(hipStream_t s, const float* x, int64_t total4, int blocks, Part* parts) {
    hipLaunchKernelGGL(bn_moments_kernel<C>, dim3(blocks), dim3(MOM_THREADS), 0, s, reinterpret_cast<const float4*>(x), total4, parts);
}

bool channels_ok(int c) { return c == 8 || c == 16 || c == 32 || c == 64 || c == 128; }      // the instantiations of bn_moments_kernel

}  // namespace

int rn_bnstats_prepare(rn_handle* h, const rn_weights* w) {
    BnStatsPlan* pl = new (std::nothrow) BnStatsPlan();
    if (!pl) {
        rn_set_error("rn_create: out of host memory");
        return RN_E_NOMEM;
    }
    h->bnstats = pl;
    int rc;
    void* p = nullptr;
    const auto add = [&](int node, int c, int64_t per_image, const float* gamma, const float* beta, float* mean, float* inv, float* shift, int* index) {
        BnSlot b;
        b.node = node;
        b.c = c;
        b.per_image = per_image;
        b.mean = mean;
        b.inv = inv;
        b.shift = shift;
        if ((rc = upload(h, gamma, c, &b.gamma)) != RN_OK) return rc;
        if (beta && (rc = upload(h, beta, c, &b.beta)) != RN_OK) return rc;
        if (!b.mean) {
            if ((rc = dev_alloc(h, static_cast<size_t>(c) * 4, &p)) != RN_OK) return rc;
            b.mean = static_cast<float*>(p);
        }
        if ((rc = dev_alloc(h, static_cast<size_t>(c) * 4, &p)) != RN_OK) return rc;
        b.var = static_cast<float*>(p);
        if ((rc = dev_alloc(h, static_cast<size_t>(c) * sizeof(double), &p)) != RN_OK) return rc;
        b.merged_n = static_cast<double*>(p);
        *index = static_cast<int>(pl->bns.size());
        pl->bns.push_back(b);
        return static_cast<int>(RN_OK);
    };
    for (size_t i = 0; i < h->stages.size(); ++i) {
        const rn_conv_stage& s = w->stages[i];
        StagePlan& sp = h->stages[i];
        if (!channels_ok(s.cout)) {
            rn_set_error("rn_create: RN_FLAG_BATCH_STATS supports 8, 16, 32, 64 or 128 channels per BN (stage %zu has %d)", i, s.cout);
            return RN_E_INVALID;
        }
        const int64_t px = static_cast<int64_t>(sp.out_side) * sp.out_side;
        int a = -1, b = -1;
        if ((rc = add(sp.node_bn, s.cout, px, s.gamma, nullptr, sp.bn.mean, sp.bn.inv, nullptr, &a)) != RN_OK) return rc;
        if (s.skip_stage >= 0 && (rc = add(sp.node_bn2, s.cout, px, s.gamma2, nullptr, sp.bn2.mean, sp.bn2.inv, nullptr, &b)) != RN_OK) return rc;
        pl->stage_bn.push_back(a);
        pl->stage_bn2.push_back(b);
    }
    for (size_t d = 0; d < h->dense.size(); ++d) {
        const rn_dense_layer& l = w->dense[d];
        DensePlan& dp = h->dense[d];
        int a = -1;
        if (l.gamma) {
            if (d + 1 == h->dense.size() || l.bias) {
                rn_set_error("rn_create: RN_FLAG_BATCH_STATS expects the normalised dense blocks without bias and a last block without BN");
                return RN_E_INVALID;
            }
            if ((rc = add(dp.node_bn, l.nout, 1, l.gamma, l.beta, nullptr, dp.inv, dp.shift, &a)) != RN_OK) return rc;
        } else if (d + 1 != h->dense.size()) {
            rn_set_error("rn_create: RN_FLAG_BATCH_STATS expects a BN behind every dense block but the last");
            return RN_E_INVALID;
        }
        pl->dense_bn.push_back(a);
    }
    if ((rc = dev_alloc(h, static_cast<size_t>(MOM_MAX_BLOCKS) * MAX_BN_CHANNELS * sizeof(Part), &p)) != RN_OK) return rc;
    pl->parts = static_cast<Part*>(p);
    return RN_OK;
}

void rn_bnstats_release(rn_handle* h) {
    delete plan_of(h);
    h->bnstats = nullptr;
}

// moments of x [npix, c] -> the table of stage `stage`'s first (second = false) or second BN
int rn_bnstats_conv(rn_handle* h, int stage, bool second, const float* x, int64_t npix) {
    BnStatsPlan* pl = plan_of(h);
    const BnSlot& b = pl->bns[second ? pl->stage_bn2[stage] : pl->stage_bn[stage]];
    const int64_t total4 = npix * b.c / 4;
    const int blocks = moments_blocks(total4);
    switch (b.c) {
        case 8: launch_moments<8>(h->stream, x, total4, blocks, pl->parts); break;
        case 16: launch_moments<16>(h->stream, x, total4, blocks, pl->parts); break;
        case 32: launch_moments<32>(h->stream, x, total4, blocks, pl->parts); break;
        case 64: launch_moments<64>(h->stream, x, total4, blocks, pl->parts); break;
        default: launch_moments<128>(h->stream, x, total4, blocks, pl->parts); break;
    }
    RN_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finalise_kernel, dim3(b.c), dim3(64), 0, h->stream, pl->parts, blocks, b.c, b.gamma, h->bn_eps, b.mean, b.var, b.inv,
                       b.merged_n);
    RN_CHECK_LAUNCH();
    return RN_OK;
}

// the head of a batch-statistics handle: per normalised block dense -> ReLU6, then moments over the batch + BN; the last block,
// softmax and argmax through head_kernel (a chain of one layer reading dK.bn of the block before it)
int rn_bnstats_head(rn_handle* h, int n, float* d_probs, int64_t* d_ids) {
    BnStatsPlan* pl = plan_of(h);
    const float* cur = static_cast<const float*>(h->nodes[h->node_flat].ptr);
    const int nd = static_cast<int>(h->dense.size());
    for (int d = 0; d + 1 < nd; ++d) {
        const DensePlan& dp = h->dense[d];
        const BnSlot& b = pl->bns[pl->dense_bn[d]];
        if (dp.nin > DENSE_MAX_IN || dp.nout > 64) {
            rn_set_error("dense layer %d (%d -> %d) exceeds the batch-statistics head's capacity (%d -> 64)", d, dp.nin, dp.nout, DENSE_MAX_IN);
            return RN_E_INVALID;
        }
        float* mm = static_cast<float*>(h->nodes[dp.node_mm].ptr);
        float* relu = static_cast<float*>(h->nodes[dp.node_relu].ptr);
        float* bn = static_cast<float*>(h->nodes[dp.node_bn].ptr);
        const int threads = (dp.nin > 256 && 1024 % dp.nout == 0) ? 1024 : 64;
        hipLaunchKernelGGL(dense_relu6_kernel, dim3(n), dim3(threads), 0, h->stream, cur, dp.w, dp.bias, dp.nin, dp.nout, mm, relu);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(dense_bn_batch_kernel, dim3(1), dim3(256), 0, h->stream, relu, n, dp.nout, b.gamma, b.beta, h->bn_eps, b.mean, b.var,
                           b.inv, b.shift, b.merged_n, bn);
        RN_CHECK_LAUNCH();
        cur = bn;
    }
    HeadArgs a;
    rn_fill_head_args(h, &a);
    HeadArgs last{};
    last.n_dense = 1;
    last.nin[0] = a.nin[nd - 1];
    last.nout[0] = a.nout[nd - 1];
    last.w[0] = a.w[nd - 1];
    last.bias[0] = a.bias[nd - 1];
    last.tap_mm[0] = a.tap_mm[nd - 1];
    last.tap_relu[0] = a.tap_relu[nd - 1];
    return rn_launch_head(h->stream, cur, RN_DTYPE_F32, n, last, d_probs, d_ids);
}

// ---- read-out of the last call's moments
namespace {
int stats_handle(const rn_handle* h, const char* who) {
    if (!h) {
        rn_set_error("%s: null handle", who);
        return RN_E_INVALID;
    }
    if (!h->bnstats) {
        rn_set_error("%s: the handle was not created with RN_FLAG_BATCH_STATS", who);
        return RN_E_STATE;
    }
    return RN_OK;
}
}  // namespace

extern "C" int rn_bn_count(const rn_handle* h) {
    int rc = stats_handle(h, "rn_bn_count");
    return rc != RN_OK ? rc : static_cast<int>(plan_of(h)->bns.size());
}

extern "C" int rn_bn_info(const rn_handle* h, int i, rn_node_info* out) {
    int rc = stats_handle(h, "rn_bn_info");
    if (rc != RN_OK) return rc;
    const BnStatsPlan* pl = plan_of(h);
    if (!out || i < 0 || i >= static_cast<int>(pl->bns.size())) {
        rn_set_error("rn_bn_info: index %d out of range (%zu BNs)", i, pl->bns.size());
        return RN_E_RANGE;
    }
    *out = h->nodes[pl->bns[i].node].info;
    return RN_OK;
}

extern "C" int rn_bn_batch_stats(rn_handle* h, int i, float* mean, float* var_biased, int64_t* count) {
    int rc = stats_handle(h, "rn_bn_batch_stats");
    if (rc != RN_OK) return rc;
    const BnStatsPlan* pl = plan_of(h);
    if (i < 0 || i >= static_cast<int>(pl->bns.size())) {
        rn_set_error("rn_bn_batch_stats: index %d out of range (%zu BNs)", i, pl->bns.size());
        return RN_E_RANGE;
    }
    if (h->last_n < 1) {
        rn_set_error("rn_bn_batch_stats: no forward pass has run on this handle");
        return RN_E_STATE;
    }
    const BnSlot& b = pl->bns[i];
    DeviceGuard guard(h->device);
    if (!guard.ok) RN_HIP(hipSetDevice(h->device));      // (fails again: reports it)
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && mean) e = hipMemcpy(mean, b.mean, static_cast<size_t>(b.c) * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && var_biased) e = hipMemcpy(var_biased, b.var, static_cast<size_t>(b.c) * 4, hipMemcpyDeviceToHost);
    double merged[MAX_BN_CHANNELS];
    if (e == hipSuccess && count) e = hipMemcpy(merged, b.merged_n, static_cast<size_t>(b.c) * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        rn_set_error("rn_bn_batch_stats: device copy failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return RN_E_HIP;
    }
    if (count) {
        // the count the device merged, not last_n * per_image: a float4 the partition dropped or read twice shows here
        // (one message for all three: a count that is no whole number in [1, 2^53), channels that differ)
        const double n0 = merged[0];
        bool ok = n0 >= 1.0 && n0 < 9.0e15 && n0 == static_cast<double>(static_cast<int64_t>(n0));
        for (int c = 1; ok && c < b.c; ++c) ok = merged[c] == n0;
        if (!ok) {
            rn_set_error("rn_bn_batch_stats: merged counts disagree");
            return RN_E_STATE;
        }
        *count = static_cast<int64_t>(n0);
    }
    return RN_OK;
}
