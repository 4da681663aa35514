// Host side of libroomnet_hip.so: execution plan, weight upload, forward orchestration,
// taps and timing.  See include/roomnet_hip.h for the contract of every entry point and
// the reference interface (file:line) it replaces.
#include "rn_internal.h"
#include "rn_fused.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

// ------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void rn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* rn_last_error(void) { return g_err; }
extern "C" const char* rn_version(void) { return RN_VERSION_STRING; }

extern "C" int rn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------ helpers
DeviceGuard::DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
}
DeviceGuard::DeviceGuard(int dev) : DeviceGuard() { ok = hipSetDevice(dev) == hipSuccess; }
DeviceGuard::~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
}

// (the failure's status is consumed: it must not come back as the "launch failure" of the thread's next kernel, see RN_HIP)
int rn_owned_alloc(std::vector<void*>& owner, size_t bytes, size_t min_bytes, void** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : min_bytes);
    if (e != hipSuccess) {
        rn_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        (void)hipGetLastError();
        return RN_E_NOMEM;
    }
    owner.push_back(p);
    *out = p;
    return RN_OK;
}

void rn_legacy_resize_table(int in_size, int out_size, int32_t* lo, int32_t* hi, float* lerp) {
    const float scale = static_cast<float>(in_size) / static_cast<float>(out_size);
    for (int i = 0; i < out_size; ++i) {
        const float src = static_cast<float>(i) * scale;
        lo[i] = static_cast<int32_t>(src);
        hi[i] = lo[i] + 1 < in_size - 1 ? lo[i] + 1 : in_size - 1;
        lerp[i] = src - static_cast<float>(lo[i]);
    }
}

int rn_stage_sides(const rn_weights* w, std::vector<int>& conv, std::vector<int>& out) {
    conv.assign(w->n_stages, 0);
    out.assign(w->n_stages, 0);
    int side = w->im_side;
    for (int i = 0; i < w->n_stages; ++i) {
        const int pool_k = w->stages[i].pool_k, pool_s = w->stages[i].pool_s;
        conv[i] = side - 2;
        if (conv[i] < 1 || (pool_k && (conv[i] < pool_k || pool_s < 1))) return i;
        out[i] = side = pool_k ? (conv[i] - pool_k) / pool_s + 1 : conv[i];
    }
    return w->n_stages;
}

int rn_lastblock_sides(const rn_weights* w, rn_lastblock* s) {
    std::vector<int> conv, out;
    const int ns = w->n_stages, fit = rn_stage_sides(w, conv, out);
    if (fit == ns && ns >= 4) *s = rn_lastblock{out[ns - 4], conv[ns - 3], out[ns - 3], conv[ns - 2], out[ns - 2], conv[ns - 1], out[ns - 1]};
    return fit;
}

void rn_lastblock_resize_tables(const rn_lastblock& s, std::vector<int32_t>& rtab, std::vector<float>& lerp) {
    rtab.resize(2 * static_cast<size_t>(s.S9));
    lerp.resize(s.S9);
    rn_legacy_resize_table(s.S7, s.S9, rtab.data(), rtab.data() + s.S9, lerp.data());
}

RelabelledWeights::RelabelledWeights(const rn_weights* src) : w(*src), stages(src->stages, src->stages + src->n_stages) {
    w.stages = stages.data();
}

void RelabelledWeights::permute_couts(int stage, const std::vector<int>& pi) {
    rn_conv_stage& st = stages[stage];
    const size_t nk = static_cast<size_t>(9) * st.cin;
    owned.emplace_back(nk * st.cout);
    for (size_t k = 0; k < nk; ++k)
        for (int co = 0; co < st.cout; ++co) owned.back()[k * st.cout + co] = st.kernel[k * st.cout + pi[co]];
    st.kernel = owned.back().data();
    const auto perm = [&](const float*& v) {
        if (!v) return;
        owned.emplace_back(pi.size());
        for (size_t p = 0; p < pi.size(); ++p) owned.back()[p] = v[pi[p]];
        v = owned.back().data();
    };
    for (const float** v : {&st.gamma, &st.beta, &st.mean, &st.variance}) perm(*v);
    if (st.skip_stage >= 0)
        for (const float** v : {&st.gamma2, &st.beta2, &st.mean2, &st.variance2}) perm(*v);
}

void RelabelledWeights::permute_cins(int stage, const std::vector<int>& pi) {
    rn_conv_stage& st = stages[stage];
    owned.emplace_back(static_cast<size_t>(9) * st.cin * st.cout);
    for (int tap = 0; tap < 9; ++tap)
        for (int ci = 0; ci < st.cin; ++ci)
            std::memcpy(&owned.back()[(static_cast<size_t>(tap) * st.cin + ci) * st.cout],
                        &st.kernel[(static_cast<size_t>(tap) * st.cin + pi[ci]) * st.cout], static_cast<size_t>(st.cout) * 4);
    st.kernel = owned.back().data();
}

void RelabelledWeights::permute_block(int r, const std::vector<int>& pi) {
    permute_couts(r - 1, pi);
    permute_couts(r, pi);
    permute_cins(r, pi);
    permute_cins(r + 1, pi);
}

bool rn_fold_block_at(const rn_weights* w, int r) {
    if (r < 1 || r + 1 >= w->n_stages) return false;
    const rn_conv_stage &s4 = w->stages[r - 1], &s5 = w->stages[r], &s6 = w->stages[r + 1];
    if (!(s5.cin == 64 && s5.cout == 64 && s5.pool_k == 4 && s5.pool_s == 2 && s5.skip_stage == r - 1 && s5.gamma2 && s4.cout == 64 &&
          s4.skip_stage < 0 && s6.cin == 64 && s6.skip_stage < 0))
        return false;
    bool other_use = false;          // nobody else may pair with the relabelled tensors
    for (int k = 0; k < w->n_stages; ++k) other_use |= (k != r && w->stages[k].skip_stage == r - 1) || w->stages[k].skip_stage == r;
    return !other_use;
}

void rn_fold_block_register(rn_handle* h, int r, const std::vector<int>& pi) {
    h->node_perm[h->stages[r - 1].node_bn] = pi;
    h->node_perm[h->stages[r].node_bn2] = pi;
}

namespace {

int upload_bn(rn_handle* h, int c, const float* gamma, const float* beta, const float* mean, const float* var,
              float eps, BnDev* out) {
    std::vector<float> inv(c);
    for (int i = 0; i < c; ++i) inv[i] = rn_bn_inv(var[i], gamma[i], eps);
    int rc;
    if ((rc = upload(h, mean, c, &out->mean)) != RN_OK) return rc;
    if ((rc = upload(h, inv.data(), c, &out->inv)) != RN_OK) return rc;
    if ((rc = upload(h, beta, c, &out->beta)) != RN_OK) return rc;
    return RN_OK;
}

int upload_resize_tab(rn_handle* h, int in_size, int out_size, ResizeTab* rt) {
    std::vector<int32_t> lo(out_size), hi(out_size);
    std::vector<float> lerp(out_size);
    rn_legacy_resize_table(in_size, out_size, lo.data(), hi.data(), lerp.data());
    int rc;
    if ((rc = upload(h, lo.data(), out_size, &rt->lo)) != RN_OK) return rc;
    if ((rc = upload(h, hi.data(), out_size, &rt->hi)) != RN_OK) return rc;
    if ((rc = upload(h, lerp.data(), out_size, &rt->lerp)) != RN_OK) return rc;
    return RN_OK;
}

int add_node(rn_handle* h, const char* name, int hh, int ww, int cc) {
    NodeBuf nb;
    std::memset(&nb.info, 0, sizeof(nb.info));
    std::snprintf(nb.info.name, RN_NAME_LEN, "%s", name);
    nb.info.h = hh;
    nb.info.w = ww;
    nb.info.c = cc;
    h->nodes.push_back(nb);
    return static_cast<int>(h->nodes.size()) - 1;
}

size_t node_elems(const NodeBuf& nb) { return static_cast<size_t>(nb.info.h) * nb.info.w * nb.info.c; }

size_t dtype_size(int dtype) { return dtype == RN_DTYPE_F32 ? 4 : 2; }

bool fused_mode(const rn_handle* h) { return h->dtype != RN_DTYPE_F32; }

int validate(const rn_weights* w, int dtype, int max_batch, unsigned flags) {
    if (!w || !w->stages || !w->dense) {
        rn_set_error("rn_create: null weights");
        return RN_E_INVALID;
    }
    if (w->n_stages < 1 || w->n_stages > RN_MAX_STAGES || w->n_dense < 1 || w->n_dense > RN_MAX_DENSE) {
        rn_set_error("rn_create: unsupported stage/dense count (%d/%d)", w->n_stages, w->n_dense);
        return RN_E_INVALID;
    }
    if (w->im_side < 8 || w->num_classes < 1 || w->num_classes > 64) {
        rn_set_error("rn_create: bad im_side %d / num_classes %d", w->im_side, w->num_classes);
        return RN_E_INVALID;
    }
    if (dtype != RN_DTYPE_F32 && dtype != RN_DTYPE_BF16 && dtype != RN_DTYPE_F16) {
        rn_set_error("rn_create: unknown dtype %d", dtype);
        return RN_E_INVALID;
    }
    if (flags & ~(RN_FLAG_TAPS | RN_FLAG_STAGE_LAUNCHES | RN_FLAG_GENERIC_KERNELS | RN_FLAG_PAIR_32X32 | RN_FLAG_COMPUTE_FROZEN | RN_FLAG_NO_DITHER | RN_FLAG_BATCH_STATS)) {
        rn_set_error("rn_create: unknown flag bits 0x%x", flags);
        return RN_E_INVALID;
    }
#ifndef RN_ROUND2_ARMS
    if (flags & RN_FLAG_PAIR_32X32) {
        rn_set_error("rn_create: RN_FLAG_PAIR_32X32 selects the round-2 comparison kernels, which are built into libroomnet_hip_ab.so "
                     "(tests and A/B runs; roomnet_amd/csrc/build.sh) and not into this library");
        return RN_E_INVALID;
    }
#endif
    if ((flags & RN_FLAG_TAPS) && dtype != RN_DTYPE_F32) {
        rn_set_error("rn_create: RN_FLAG_TAPS needs RN_DTYPE_F32 (the unfused per-node path)");
        return RN_E_INVALID;
    }
    if (flags & RN_FLAG_BATCH_STATS) {
        if (dtype != RN_DTYPE_F32) {
            rn_set_error("rn_create: RN_FLAG_BATCH_STATS needs RN_DTYPE_F32 (batch moments run on the float32 per-node path)");
            return RN_E_INVALID;
        }
        if (flags & (RN_FLAG_GENERIC_KERNELS | RN_FLAG_STAGE_LAUNCHES | RN_FLAG_PAIR_32X32)) {
            rn_set_error("rn_create: RN_FLAG_BATCH_STATS does not combine with the 16-bit handles' flags (0x%x)",
                         flags & (RN_FLAG_GENERIC_KERNELS | RN_FLAG_STAGE_LAUNCHES | RN_FLAG_PAIR_32X32));
            return RN_E_INVALID;
        }
    }
    if (max_batch < 1) {
        rn_set_error("rn_create: max_batch must be >= 1");
        return RN_E_INVALID;
    }
    if (w->stages[0].cin != 3) {
        rn_set_error("rn_create: first stage must take 3 input channels");
        return RN_E_INVALID;
    }
    return RN_OK;
}

int build_plan(rn_handle* h, const rn_weights* w) {
    int side = w->im_side, ch = 3, rc;
    h->node_input = add_node(h, "input", side, side, 3);
    char name[RN_NAME_LEN];
    std::vector<int> conv_side, out_side;
    const int n_fit = rn_stage_sides(w, conv_side, out_side);
    for (int i = 0; i < w->n_stages; ++i) {
        const rn_conv_stage& s = w->stages[i];
        if (s.cin != ch || s.cout < 1 || s.cout > 512 || !s.kernel || !s.gamma || !s.beta || !s.mean ||
            !s.variance) {
            rn_set_error("stage %d: inconsistent description (cin %d, expected %d)", i, s.cin, ch);
            return RN_E_INVALID;
        }
        StagePlan p{};
        p.cin = s.cin;
        p.cout = s.cout;
        p.in_side = side;
        p.pool_k = s.pool_k;
        p.pool_s = s.pool_k ? s.pool_s : 1;
        if (i >= n_fit) {
            rn_set_error("stage %d: im_side too small for this graph", i);
            return RN_E_INVALID;
        }
        p.conv_side = conv_side[i];
        p.out_side = out_side[i];
        p.skip_stage = s.skip_stage;
        if (s.skip_stage >= 0) {
            if (s.skip_stage >= i || h->stages[s.skip_stage].cout != s.cout || !s.gamma2 || !s.beta2 ||
                !s.mean2 || !s.variance2) {
                rn_set_error("stage %d: bad residual description", i);
                return RN_E_INVALID;
            }
            p.skip_side = h->stages[s.skip_stage].out_side;
        }
        if ((rc = upload(h, s.kernel, static_cast<size_t>(9) * s.cin * s.cout, &p.w_f32)) != RN_OK) return rc;
        if ((rc = upload_bn(h, s.cout, s.gamma, s.beta, s.mean, s.variance, w->bn_epsilon, &p.bn)) != RN_OK)
            return rc;
        if (s.skip_stage >= 0) {
            if ((rc = upload_bn(h, s.cout, s.gamma2, s.beta2, s.mean2, s.variance2, w->bn_epsilon, &p.bn2)) !=
                RN_OK)
                return rc;
            if ((rc = upload_resize_tab(h, p.skip_side, p.out_side, &p.rt)) != RN_OK) return rc;
        }
        std::snprintf(name, sizeof(name), "s%d.conv", i);
        p.node_conv = add_node(h, name, p.conv_side, p.conv_side, p.cout);
        if (p.pool_k) {
            std::snprintf(name, sizeof(name), "s%d.pool", i);
            p.node_pool = add_node(h, name, p.out_side, p.out_side, p.cout);
        }
        std::snprintf(name, sizeof(name), "s%d.bn", i);
        p.node_bn = add_node(h, name, p.out_side, p.out_side, p.cout);
        if (s.skip_stage >= 0) {
            std::snprintf(name, sizeof(name), "s%d.add", i);
            p.node_add = add_node(h, name, p.out_side, p.out_side, p.cout);
            std::snprintf(name, sizeof(name), "s%d.bn2", i);
            p.node_bn2 = add_node(h, name, p.out_side, p.out_side, p.cout);
        }
        h->stages.push_back(p);
        side = p.out_side;
        ch = p.cout;
    }
    const int flat_len = side * side * ch;
    h->node_flat = add_node(h, "flat", 1, 1, flat_len);
    int nin = flat_len;
    for (int d = 0; d < w->n_dense; ++d) {
        const rn_dense_layer& l = w->dense[d];
        if (l.nin != nin || l.nout < 1 || l.nout > 64 || !l.kernel) {
            rn_set_error("dense %d: expected %d inputs, got %d (is the checkpoint for this im_side?)", d, nin,
                         l.nin);
            return RN_E_INVALID;
        }
        DensePlan p{};
        p.nin = l.nin;
        p.nout = l.nout;
        if ((rc = upload(h, l.kernel, static_cast<size_t>(l.nin) * l.nout, &p.w)) != RN_OK) return rc;
        if (l.bias && (rc = upload(h, l.bias, l.nout, &p.bias)) != RN_OK) return rc;
        if (l.gamma) {
            if (!l.beta || !l.mean || !l.variance) {
                rn_set_error("dense %d: incomplete BN parameters", d);
                return RN_E_INVALID;
            }
            // tf.nn.batch_normalization: inv = rsqrt(var+eps)*gamma; shift = beta - mean*inv
            std::vector<float> inv(l.nout), shift(l.nout);
            for (int j = 0; j < l.nout; ++j) {
                inv[j] = rn_bn_inv(l.variance[j], l.gamma[j], w->bn_epsilon);
                shift[j] = rn_bn_shift(l.beta[j], l.mean[j], inv[j]);
            }
            if ((rc = upload(h, inv.data(), l.nout, &p.inv)) != RN_OK) return rc;
            if ((rc = upload(h, shift.data(), l.nout, &p.shift)) != RN_OK) return rc;
        }
        std::snprintf(name, sizeof(name), "d%d.mm", d);
        p.node_mm = add_node(h, name, 1, 1, l.nout);
        std::snprintf(name, sizeof(name), "d%d.relu", d);
        p.node_relu = add_node(h, name, 1, 1, l.nout);
        if (l.gamma) {
            std::snprintf(name, sizeof(name), "d%d.bn", d);
            p.node_bn = add_node(h, name, 1, 1, l.nout);
        }
        h->dense.push_back(p);
        nin = l.nout;
    }
    if (nin != w->num_classes) {
        rn_set_error("last dense layer has %d outputs, num_classes is %d", nin, w->num_classes);
        return RN_E_INVALID;
    }
    h->node_softmax = add_node(h, "softmax", 1, 1, w->num_classes);
    return RN_OK;
}

// Allocate activation buffers.  Stage outputs always get their own buffer (they are
// skip sources and are always tappable).  In the unfused path the conv/pool/add
// intermediates share two scratch buffers unless RN_FLAG_TAPS asks for all of them.
int alloc_buffers(rn_handle* h) {
    const size_t nb = static_cast<size_t>(h->max_batch);
    int rc;
    const bool taps = (h->flags & RN_FLAG_TAPS) != 0;
    const bool fused = fused_mode(h);
    void* p = nullptr;
    // input (fp32 RGB): unfused path only; the fused stage 0 reads uint8 directly
    if (!fused) {
        if ((rc = dev_alloc(h, nb * node_elems(h->nodes[h->node_input]) * 4, &p)) != RN_OK) return rc;
        h->nodes[h->node_input].ptr = p;
    }
    size_t scratch_elems = 0;
    for (auto& s : h->stages) {
        const int out_node = rn_stage_out_node(s);
        for (int id : {s.node_conv, s.node_pool, s.node_bn, s.node_add, s.node_bn2}) {
            if (id < 0) continue;
            NodeBuf& n = h->nodes[id];
            const bool is_out = (id == out_node) || (id == s.node_bn);
            if (fused) {
                if (id == out_node) {
                    n.dtype = h->dtype;
                    if ((rc = dev_alloc(h, nb * node_elems(n) * dtype_size(h->dtype) + 8192, &p)) != RN_OK) return rc;
                    n.ptr = p;
                }
                continue;
            }
            if (taps || is_out) {
                if ((rc = dev_alloc(h, nb * node_elems(n) * 4, &p)) != RN_OK) return rc;
                n.ptr = p;
            } else {
                scratch_elems = std::max(scratch_elems, node_elems(n));
            }
        }
    }
    if (!fused && !taps) {
        void* s0 = nullptr;
        void* s1 = nullptr;
        if ((rc = dev_alloc(h, nb * scratch_elems * 4, &s0)) != RN_OK) return rc;
        if ((rc = dev_alloc(h, nb * scratch_elems * 4, &s1)) != RN_OK) return rc;
        for (auto& s : h->stages) {
            if (s.node_conv >= 0 && !h->nodes[s.node_conv].ptr) h->nodes[s.node_conv].ptr = s0;
            if (s.node_pool >= 0 && !h->nodes[s.node_pool].ptr) h->nodes[s.node_pool].ptr = s1;
            if (s.node_add >= 0 && !h->nodes[s.node_add].ptr) h->nodes[s.node_add].ptr = s0;
        }
    }
    // flat aliases the last stage output
    {
        const StagePlan& last = h->stages.back();
        const NodeBuf& src = h->nodes[rn_stage_out_node(last)];
        h->nodes[h->node_flat].ptr = src.ptr;
        h->nodes[h->node_flat].dtype = src.dtype;
    }
    for (auto& d : h->dense)
        for (int id : {d.node_mm, d.node_relu, d.node_bn}) {
            if (id < 0) continue;
            if ((rc = dev_alloc(h, nb * node_elems(h->nodes[id]) * 4, &p)) != RN_OK) return rc;
            h->nodes[id].ptr = p;
        }
    // staging for the host-buffer entry points + softmax node
    if ((rc = dev_alloc(h, nb * h->im_side * h->im_side * 3, &p)) != RN_OK) return rc;
    h->d_in_u8 = static_cast<uint8_t*>(p);
    if ((rc = dev_alloc(h, nb * h->num_classes * 4, &p)) != RN_OK) return rc;
    h->d_probs = static_cast<float*>(p);
    h->nodes[h->node_softmax].ptr = p;
    if ((rc = dev_alloc(h, nb * 8, &p)) != RN_OK) return rc;
    h->d_ids = static_cast<int64_t*>(p);
    return RN_OK;
}

void record(rn_handle* h, int idx) {
    if (h->profiling && idx < static_cast<int>(h->events.size())) (void)hipEventRecord(h->events[idx], h->stream);
}

void fill_head_args(rn_handle* h, HeadArgs& a) {
    a = HeadArgs{};
    a.n_dense = static_cast<int>(h->dense.size());
    for (int d = 0; d < a.n_dense; ++d) {
        const DensePlan& p = h->dense[d];
        a.nin[d] = p.nin;
        a.nout[d] = p.nout;
        a.w[d] = p.w;
        a.bias[d] = p.bias;
        a.inv[d] = p.inv;
        a.shift[d] = p.shift;
        a.tap_mm[d] = static_cast<float*>(h->nodes[p.node_mm].ptr);
        a.tap_relu[d] = static_cast<float*>(h->nodes[p.node_relu].ptr);
        a.tap_bn[d] = p.node_bn >= 0 ? static_cast<float*>(h->nodes[p.node_bn].ptr) : nullptr;
    }
}

int run_head(rn_handle* h, int n, float* d_probs, int64_t* d_ids) {
    HeadArgs a;
    fill_head_args(h, a);
    // the features lie in front of the head: a handle whose flatten head_kernel cannot take (im_side > 694) still serves them, with
    // no head launch and nothing written to the head's nodes; every classifying call is refused by rn_launch_head
    if (h->features_pass && !rn_head_takes_flatten(a.nin[0])) return RN_OK;
    const NodeBuf& flat = h->nodes[h->node_flat];
    return rn_launch_head(h->stream, flat.ptr, flat.dtype, n, a, d_probs, d_ids);
}

// Float32 forward: one launch per graph node; without RN_FLAG_TAPS the conv stages rn_stage_f32m.hip covers run as one
// matrix-core launch each.
int forward_unfused(rn_handle* h, const float* d_rgb, int n, float* d_probs, int64_t* d_ids) {
    int rc;
    const float* cur = d_rgb;
    for (size_t i = 0; i < h->stages.size(); ++i) {
        StagePlan& s = h->stages[i];
        if (rn_f32m_covers(h, static_cast<int>(i))) {
            // the whole stage in one launch on the matrix cores; only its output node is written
            if ((rc = rn_f32m_launch(h, static_cast<int>(i), n)) != RN_OK) return rc;
            cur = static_cast<const float*>(h->nodes[rn_stage_out_node(s)].ptr);
            record(h, 2 + static_cast<int>(i));
            continue;
        }
        if (i == 0 && h->f32m && s.cin == 3 && s.cout == 8 && s.pool_k == 3 && s.pool_s == 1 && s.skip_stage < 0) {
            // (handles without taps) stage 0 in one launch, bit-identical to its per-node launches
            float* bn0 = static_cast<float*>(h->nodes[s.node_bn].ptr);
            if ((rc = rn_launch_stage0_fused_f32(h->stream, cur, s.w_f32, bn0, n, s.in_side, s.bn)) != RN_OK) return rc;
            cur = bn0;
            record(h, 2 + static_cast<int>(i));
            continue;
        }
        float* conv = static_cast<float*>(h->nodes[s.node_conv].ptr);
        if ((rc = rn_launch_conv3x3_relu6_f32(h->stream, cur, s.w_f32, conv, n, s.in_side, s.in_side, s.cin,
                                              s.cout)) != RN_OK)
            return rc;
        const float* pooled = conv;
        if (s.pool_k) {
            float* pl = static_cast<float*>(h->nodes[s.node_pool].ptr);
            if ((rc = rn_launch_avgpool_f32(h->stream, conv, pl, n, s.conv_side, s.conv_side, s.cout, s.pool_k,
                                            s.pool_s)) != RN_OK)
                return rc;
            pooled = pl;
        }
        float* bn = static_cast<float*>(h->nodes[s.node_bn].ptr);
        const int64_t npix = static_cast<int64_t>(n) * s.out_side * s.out_side;
        // (batch-statistics handles: the table s.bn is written on the device from this tensor's moments first)
        if (h->bnstats && (rc = rn_bnstats_conv(h, static_cast<int>(i), false, pooled, npix)) != RN_OK) return rc;
        if ((rc = rn_launch_bn_f32(h->stream, pooled, bn, npix, s.cout, s.bn)) != RN_OK) return rc;
        cur = bn;
        if (s.skip_stage >= 0) {
            const StagePlan& sk = h->stages[s.skip_stage];
            const float* skip = static_cast<const float*>(h->nodes[sk.node_bn].ptr);
            float* add = static_cast<float*>(h->nodes[s.node_add].ptr);
            if ((rc = rn_launch_resize_add_f32(h->stream, bn, skip, add, n, s.out_side, s.skip_side, s.cout,
                                               s.rt)) != RN_OK)
                return rc;
            float* bn2 = static_cast<float*>(h->nodes[s.node_bn2].ptr);
            if (h->bnstats && (rc = rn_bnstats_conv(h, static_cast<int>(i), true, add, npix)) != RN_OK) return rc;
            if ((rc = rn_launch_bn_f32(h->stream, add, bn2, npix, s.cout, s.bn2)) != RN_OK) return rc;
            cur = bn2;
        }
        record(h, 2 + static_cast<int>(i));
    }
    if ((rc = h->bnstats ? rn_bnstats_head(h, n, d_probs, d_ids) : run_head(h, n, d_probs, d_ids)) != RN_OK) return rc;
    record(h, 2 + static_cast<int>(h->stages.size()));
    return RN_OK;
}

int check_call(rn_handle* h, int n, const void* a, const void* b, const void* c) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    if (!a || !b || !c) {
        rn_set_error("null buffer");
        return RN_E_INVALID;
    }
    if (n < 1 || n > h->max_batch) {
        rn_set_error("batch %d out of range (max_batch %d)", n, h->max_batch);
        return RN_E_RANGE;
    }
    return RN_OK;
}

// the kernels are gfx950 code sized for its 160 KiB of LDS per CU: refuse anything else up front
int check_device(int device, int* n_cu) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        rn_set_error("rn_create: no HIP device available");
        return RN_E_HIP;
    }
    if (device < 0 || device >= ndev) {
        rn_set_error("rn_create: device %d out of range (%d devices)", device, ndev);
        return RN_E_INVALID;
    }
    hipDeviceProp_t prop{};
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        rn_set_error("rn_create: hipGetDeviceProperties(%d) failed", device);
        return RN_E_HIP;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 || prop.maxSharedMemoryPerMultiProcessor < 160 * 1024) {
        rn_set_error("rn_create: device %d is %s with %zu bytes of LDS per CU; this library is built for gfx950 (MI355X, 160 KiB)",
                     device, prop.gcnArchName, static_cast<size_t>(prop.maxSharedMemoryPerMultiProcessor));
        return RN_E_INVALID;
    }
    *n_cu = prop.multiProcessorCount;
    return RN_OK;
}

}  // namespace

int rn_run_head(rn_handle* h, int n, float* d_probs, int64_t* d_ids) { return run_head(h, n, d_probs, d_ids); }
void rn_fill_head_args(rn_handle* h, HeadArgs* a) { fill_head_args(h, *a); }
void rn_record_event(rn_handle* h, int idx) { record(h, idx); }

// ---------------------------------------------------------------------------- API
extern "C" int rn_create(const rn_weights* w, int device, int dtype, int max_batch, unsigned flags,
                         rn_handle** out) {
    if (!out) {
        rn_set_error("rn_create: null out pointer");
        return RN_E_INVALID;
    }
    *out = nullptr;
    int rc = validate(w, dtype, max_batch, flags);
    if (rc != RN_OK) return rc;
    int n_cu = 0;
    if ((rc = check_device(device, &n_cu)) != RN_OK) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) {
        rn_set_error("rn_create: hipSetDevice(%d) failed", device);
        return RN_E_HIP;
    }
    rn_handle* h = new (std::nothrow) rn_handle();
    if (!h) {
        rn_set_error("rn_create: out of host memory");
        return RN_E_NOMEM;
    }
    h->n_cu = n_cu;
    h->device = device;
    h->dtype = dtype;
    h->flags = flags;
    h->max_batch = max_batch;
    h->im_side = w->im_side;
    h->num_classes = w->num_classes;
    h->bn_eps = w->bn_epsilon;
    auto fail = [&](int code) {
        rn_destroy(h);
        return code;
    };
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        rn_set_error("rn_create: hipStreamCreate failed");
        return fail(RN_E_HIP);
    }
    h->stream = h->own_stream;
    RelabelledWeights rw(w);
    const auto folds = rn_f32m_plan_folds(w, dtype, flags, &rw);      // (float32 handles: the frozen-channel folds, relabelled on rw)
    // (the grad-CAM adjoint keeps its host copies from the caller's weights, in the reference's channel order)
    if ((rc = rn_gradcam_keep(h, w)) != RN_OK) return fail(rc);
    w = &rw.w;
    if ((rc = build_plan(h, w)) != RN_OK) return fail(rc);
    // uint8 -> float32 table, evaluated in float64 like the reference's NumPy expression
    {
        float lut[256];
        for (int v = 0; v < 256; ++v) lut[v] = static_cast<float>(((static_cast<double>(v) / 255.) * 2) - 1);
        if ((rc = upload(h, lut, 256, &h->lut)) != RN_OK) return fail(rc);
    }
    if (fused_mode(h) && (rc = rn_fused_prepare(h, w)) != RN_OK) return fail(rc);
    // float32 handles without per-node taps run their conv stages on the matrix cores (rn_stage_f32m.hip)
    // (not the batch-statistics handles: their BN tables do not exist before the stage's input has been reduced)
    if (!fused_mode(h) && !(h->flags & (RN_FLAG_TAPS | RN_FLAG_BATCH_STATS)) && (rc = rn_f32m_prepare(h, w, folds)) != RN_OK)
        return fail(rc);
    if ((h->flags & RN_FLAG_BATCH_STATS) && (rc = rn_bnstats_prepare(h, w)) != RN_OK) return fail(rc);
    if ((rc = alloc_buffers(h)) != RN_OK) return fail(rc);
    if ((rc = fused_mode(h) ? rn_fused_post_alloc(h) : rn_f32m_post_alloc(h)) != RN_OK) return fail(rc);
    h->events.resize(3 + h->stages.size());
    for (auto& e : h->events)
        if (hipEventCreate(&e) != hipSuccess) {
            rn_set_error("rn_create: hipEventCreate failed");
            return fail(RN_E_HIP);
        }
    if (hipDeviceSynchronize() != hipSuccess) {
        rn_set_error("rn_create: device synchronize failed");
        return fail(RN_E_HIP);
    }
    *out = h;
    return RN_OK;
}

extern "C" void rn_destroy(rn_handle* h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    for (auto e : h->events)
        if (e) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->d_raw) (void)hipFree(h->d_raw);
    for (auto& sl : h->slots) {
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_probs) (void)hipFree(sl.d_probs);
        if (sl.d_ids) (void)hipFree(sl.d_ids);
        if (sl.h_probs) (void)hipHostFree(sl.h_probs);
        if (sl.h_ids) (void)hipHostFree(sl.h_ids);
        if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    rn_fused_release(h);
    rn_f32m_release(h);
    rn_gradcam_release(h);
    rn_bnstats_release(h);
    rn_jpeg_release(h);
    rn_jpeg_enc_release(h);
    rn_jpeg_huffenc_release(h);
    rn_cam_overlay_release(h);
    rn_occlusion_release(h);
    rn_faith_release(h);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

extern "C" int rn_set_stream(rn_handle* h, void* hip_stream) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    return RN_OK;
}

extern "C" int rn_set_stream_null(rn_handle* h) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    h->stream = nullptr;          // hipStream_t(0): the null stream
    return RN_OK;
}

extern "C" int rn_sync(rn_handle* h) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

// One forward pass on a device input: exactly one of d_bgr (uint8 BGR) / d_rgb (pre-processed float32) is given.
static int forward_device(rn_handle* h, const uint8_t* d_bgr, const float* d_rgb, int n, float* d_probs, int64_t* d_ids) {
    int rc = check_call(h, n, d_bgr ? static_cast<const void*>(d_bgr) : d_rgb, d_probs, d_ids);
    if (rc != RN_OK) return rc;
    DeviceGuard guard(h->device);
    (void)hipGetLastError();      // a stale status of the CALLER's own runtime calls on this thread is not this pass's launch failure
    h->timing_valid = false;
    record(h, 0);
    // events 0 .. 1 bracket the pre-processing: only the unfused uint8 pass has a launch of its own for it
    if (fused_mode(h)) {
        record(h, 1);
        rc = rn_fused_forward(h, d_bgr, d_rgb, n, d_probs, d_ids);
    } else {
        float* in_node = static_cast<float*>(h->nodes[h->node_input].ptr);
        if (d_bgr) {
            rc = rn_launch_preprocess_u8(h->stream, d_bgr, in_node, h->lut, static_cast<int64_t>(n) * h->im_side * h->im_side);
            if (rc != RN_OK) return rc;
            record(h, 1);
        } else {
            record(h, 1);
            // keep the "input" node readable through rn_tap
            if (in_node != d_rgb)
                RN_HIP(hipMemcpyAsync(in_node, d_rgb, static_cast<size_t>(n) * h->im_side * h->im_side * 3 * 4,
                                      hipMemcpyDeviceToDevice, h->stream));
        }
        rc = forward_unfused(h, in_node, n, d_probs, d_ids);
    }
    if (rc != RN_OK) return rc;
    h->last_n = n;
    h->timing_valid = h->profiling;
    return RN_OK;
}

extern "C" int rn_forward_f32_device(rn_handle* h, const float* d_rgb, int n, float* d_probs, int64_t* d_ids) {
    return forward_device(h, nullptr, d_rgb, n, d_probs, d_ids);
}

extern "C" int rn_forward_u8_device(rn_handle* h, const uint8_t* d_bgr, int n, float* d_probs, int64_t* d_ids) {
    return forward_device(h, d_bgr, nullptr, n, d_probs, d_ids);
}

// the tail of the host entry points: the call's probabilities and classes (h->d_probs, h->d_ids) to the caller, one synchronisation
int rn_results_to_host(rn_handle* h, int n, float* probs, int64_t* ids) {
    RN_HIP(hipMemcpyAsync(probs, h->d_probs, static_cast<size_t>(n) * h->num_classes * 4, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipMemcpyAsync(ids, h->d_ids, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

extern "C" int rn_forward_u8(rn_handle* h, const uint8_t* bgr, int n, float* probs, int64_t* ids) {
    int rc = check_call(h, n, bgr, probs, ids);
    if (rc != RN_OK) return rc;
    DeviceGuard guard(h->device);
    const size_t in_bytes = static_cast<size_t>(n) * h->im_side * h->im_side * 3;
    RN_HIP(hipMemcpyAsync(h->d_in_u8, bgr, in_bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = rn_forward_u8_device(h, h->d_in_u8, n, h->d_probs, h->d_ids)) != RN_OK) return rc;
    return rn_results_to_host(h, n, probs, ids);
}

// ---- grad-CAM class-evidence maps (rn_gradcam.hip): the forward pass of the call (16-bit handles: the back end as its split
// launches, so that s6.bn and s7.bn reach HBM), then the adjoint of the last conv block and the head
namespace {
// The shared front of the grad-CAM and the feature entry points (`name`): a handle of the inference graph whose last block the
// adjoint kernels walk, and n inside the handle's batch.  `what` is the entry point's product, for the RN_FLAG_BATCH_STATS refusal;
// `range_rc` what n out of range returns (grad-CAM: RN_E_INVALID, features: RN_E_RANGE).
int last_block_check(const rn_handle* h, int n, const char* name, const char* what, int range_rc) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    if (h->bnstats) {
        rn_set_error("%s: %s of the inference graph; this handle normalises with batch moments (RN_FLAG_BATCH_STATS)", name, what);
        return RN_E_STATE;
    }
    if (const char* why = rn_gradcam_unsupported(h)) {
        rn_set_error("%s: not supported on this graph (%s)", name, why);
        return RN_E_INVALID;
    }
    if (n < 1 || n > h->max_batch) {
        rn_set_error("%s: n = %d out of range (1..%d)", name, n, h->max_batch);
        return range_rc;
    }
    return RN_OK;
}

int gradcam_check(rn_handle* h, int n, int layer_node, bool* layer6) {
    int rc = last_block_check(h, n, "rn_grad_cam", "the adjoint is that", RN_E_INVALID);
    if (rc != RN_OK) return rc;
    int node6, node7;
    rn_gradcam_layers(h, &node6, &node7);
    if (layer_node != node6 && layer_node != node7) {
        const char* nm = layer_node >= 0 && layer_node < static_cast<int>(h->nodes.size()) ? h->nodes[layer_node].info.name : "?";
        rn_set_error("rn_grad_cam: layer node %d (%s) is not supported (s6.bn = %d, s7.bn = %d)", layer_node, nm, node6, node7);
        return RN_E_INVALID;
    }
    *layer6 = layer_node == node6;
    return RN_OK;
}

int gradcam_check_classes(rn_handle* h, const int32_t* cls, int n) {
    for (int i = 0; i < n; ++i)
        if (cls[i] < 0 || cls[i] >= h->num_classes) {
            rn_set_error("rn_grad_cam: class_ids[%d] = %d outside [0, %d)", i, cls[i], h->num_classes);
            return RN_E_INVALID;
        }
    return RN_OK;
}

// forward on the device input (exactly one of d_bgr / d_rgb), then the adjoint; classes already validated
int gradcam_device(rn_handle* h, const uint8_t* d_bgr, const float* d_rgb, int n, const int32_t* d_cls, bool layer6, float* d_cam,
                   float* d_alpha, float* d_probs, int64_t* d_ids) {
    h->split_backend = true;
    int rc = d_bgr ? rn_forward_u8_device(h, d_bgr, n, d_probs, d_ids) : rn_forward_f32_device(h, d_rgb, n, d_probs, d_ids);
    h->split_backend = false;
    if (rc != RN_OK) return rc;
    DeviceGuard guard(h->device);
    for (int s = 0; s < static_cast<int>(h->stages.size()); ++s)
        if (fused_mode(h) && rn_fused_stage_elided(h, s)) {
            int node6, node7;
            rn_gradcam_layers(h, &node6, &node7);
            if (h->stages[s].node_bn == node6 || h->stages[s].node_bn == node7) {
                rn_set_error("rn_grad_cam: the forward pass did not write %s", h->nodes[h->stages[s].node_bn].info.name);
                return RN_E_STATE;
            }
        }
    return rn_gradcam_launch(h, n, d_cls, d_ids, layer6, d_cam, d_alpha);
}

int gradcam_host(rn_handle* h, const uint8_t* bgr, const float* rgb, int n, const int32_t* class_ids, int layer_node, float* cam,
                 float* alpha, float* probs, int64_t* ids) {
    bool layer6 = false;
    int rc = gradcam_check(h, n, layer_node, &layer6);
    if (rc != RN_OK) return rc;
    if ((!bgr && !rgb) || !cam || !probs || !ids) {
        rn_set_error("null buffer");
        return RN_E_INVALID;
    }
    if (class_ids && (rc = gradcam_check_classes(h, class_ids, n)) != RN_OK) return rc;
    DeviceGuard guard(h->device);
    int32_t* d_cls = nullptr;
    float *d_cam = nullptr, *d_alpha = nullptr;
    if ((rc = rn_gradcam_staging(h, &d_cls, &d_cam, &d_alpha)) != RN_OK) return rc;
    const size_t px = static_cast<size_t>(h->im_side) * h->im_side * 3;
    if (bgr)
        RN_HIP(hipMemcpyAsync(h->d_in_u8, bgr, static_cast<size_t>(n) * px, hipMemcpyHostToDevice, h->stream));
    else if (!fused_mode(h))
        RN_HIP(hipMemcpyAsync(h->nodes[h->node_input].ptr, rgb, static_cast<size_t>(n) * px * 4, hipMemcpyHostToDevice, h->stream));
    else {
        rn_set_error("16-bit handles take uint8 BGR input (the pre-processing is folded into stage 0's weights)");
        return RN_E_STATE;
    }
    if (class_ids) RN_HIP(hipMemcpyAsync(d_cls, class_ids, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice, h->stream));
    rc = gradcam_device(h, bgr ? h->d_in_u8 : nullptr, bgr ? nullptr : static_cast<const float*>(h->nodes[h->node_input].ptr), n,
                        class_ids ? d_cls : nullptr, layer6, d_cam, d_alpha, h->d_probs, h->d_ids);
    if (rc != RN_OK) return rc;
    const rn_node_info& li = h->nodes[layer_node].info;
    RN_HIP(hipMemcpyAsync(cam, d_cam, static_cast<size_t>(n) * li.h * li.w * 4, hipMemcpyDeviceToHost, h->stream));
    if (alpha) RN_HIP(hipMemcpyAsync(alpha, d_alpha, static_cast<size_t>(n) * li.c * 4, hipMemcpyDeviceToHost, h->stream));
    return rn_results_to_host(h, n, probs, ids);
}
}  // namespace

extern "C" int rn_grad_cam_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, const int32_t* class_ids, int layer_node, float* cam,
                              float* alpha, float* probs, int64_t* ids) {
    return gradcam_host(h, bgr_nhwc, nullptr, n, class_ids, layer_node, cam, alpha, probs, ids);
}

extern "C" int rn_grad_cam_f32(rn_handle* h, const float* rgb_nhwc, int n, const int32_t* class_ids, int layer_node, float* cam,
                               float* alpha, float* probs, int64_t* ids) {
    return gradcam_host(h, nullptr, rgb_nhwc, n, class_ids, layer_node, cam, alpha, probs, ids);
}

extern "C" int rn_grad_cam_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, const int32_t* d_class_ids, int layer_node,
                                     float* d_cam, float* d_alpha, float* d_probs, int64_t* d_ids) {
    bool layer6 = false;
    int rc = gradcam_check(h, n, layer_node, &layer6);
    if (rc != RN_OK) return rc;
    if (!d_bgr_nhwc || !d_cam || !d_probs || !d_ids) {
        rn_set_error("null buffer");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    if (d_class_ids) {
        // (validated before anything is launched: the classes are read back on the handle's stream)
        std::vector<int32_t> cls(static_cast<size_t>(n));
        RN_HIP(hipMemcpyAsync(cls.data(), d_class_ids, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, h->stream));
        RN_HIP(hipStreamSynchronize(h->stream));
        if ((rc = gradcam_check_classes(h, cls.data(), n)) != RN_OK) return rc;
    }
    return gradcam_device(h, d_bgr_nhwc, nullptr, n, d_class_ids, layer6, d_cam, d_alpha, d_probs, d_ids);
}

// ---- feature read-out for the fine-tuning cache (rn_finetune.hip): a forward pass that leaves s7.bn (depth 2) or s6.bn (depth 3)
// in HBM, widened to float32
namespace {
int features_depth_check(int depth) {
    if (depth == 2 || depth == 3) return RN_OK;
    rn_set_error("rn_features_depth: depth = %d is neither 2 (s7.bn) nor 3 (s6.bn)", depth);
    return RN_E_INVALID;
}

// the node the features of `depth` are read from: s7.bn (2) or s6.bn (3)
int features_check(rn_handle* h, int n, int* node, int depth) {
    int rc = features_depth_check(depth);
    if (rc == RN_OK) rc = last_block_check(h, n, "rn_features", "the cached features are those", RN_E_RANGE);
    if (rc != RN_OK) return rc;
    int node6, node7;
    rn_gradcam_layers(h, &node6, &node7);
    *node = depth == 3 ? node6 : node7;
    return RN_OK;
}

int features_device(rn_handle* h, const uint8_t* d_bgr, int n, int node7, float* d_feat) {
    h->split_backend = h->features_pass = true;
    int rc = rn_forward_u8_device(h, d_bgr, n, h->d_probs, h->d_ids);
    h->split_backend = h->features_pass = false;
    if (rc != RN_OK) return rc;
    const NodeBuf& nb = h->nodes[node7];
    bool elided = false;
    for (int s = 0; s < static_cast<int>(h->stages.size()); ++s)
        elided |= fused_mode(h) && h->stages[s].node_bn == node7 && rn_fused_stage_elided(h, s);
    if (!nb.ptr || elided || h->node_perm.count(node7)) {
        rn_set_error("rn_features: the forward pass did not write %s in the reference's layout", nb.info.name);
        return RN_E_STATE;
    }
    DeviceGuard guard(h->device);
    const int64_t total = static_cast<int64_t>(n) * nb.info.h * nb.info.w * nb.info.c;
    if (nb.dtype == RN_DTYPE_F32) {
        RN_HIP(hipMemcpyAsync(d_feat, nb.ptr, static_cast<size_t>(total) * 4, hipMemcpyDeviceToDevice, h->stream));
        return RN_OK;
    }
    return rn_launch_convert_to_f32(h->stream, nb.ptr, nb.dtype, d_feat, total);
}
}  // namespace

extern "C" int rn_features_depth_shape(const rn_handle* h, int depth, int* side, int* channels) {
    int rc = features_depth_check(depth);
    if (rc != RN_OK) return rc;
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    if (const char* why = rn_gradcam_unsupported(h)) {
        rn_set_error("rn_features: not supported on this graph (%s)", why);
        return RN_E_INVALID;
    }
    int node6, node7;
    rn_gradcam_layers(h, &node6, &node7);
    const rn_node_info& li = h->nodes[depth == 3 ? node6 : node7].info;
    if (side) *side = li.h;
    if (channels) *channels = li.c;
    return RN_OK;
}

extern "C" int rn_features_shape(const rn_handle* h, int* side, int* channels) { return rn_features_depth_shape(h, 2, side, channels); }

extern "C" int rn_features_depth_u8_device(rn_handle* h, int depth, const uint8_t* d_bgr_nhwc, int n, float* d_feat) {
    int node = -1;
    int rc = features_check(h, n, &node, depth);
    if (rc != RN_OK) return rc;
    if (!d_bgr_nhwc || !d_feat) {
        rn_set_error("null buffer");
        return RN_E_INVALID;
    }
    return features_device(h, d_bgr_nhwc, n, node, d_feat);
}

extern "C" int rn_features_u8_device(rn_handle* h, const uint8_t* d_bgr_nhwc, int n, float* d_feat) {
    return rn_features_depth_u8_device(h, 2, d_bgr_nhwc, n, d_feat);
}

namespace {
int features_host(rn_handle* h, int depth, const uint8_t* bgr_nhwc, int n, float* feat) {
    int node = -1;
    int rc = features_check(h, n, &node, depth);
    if (rc != RN_OK) return rc;
    if (!bgr_nhwc || !feat) {
        rn_set_error("null buffer");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    const rn_node_info& li = h->nodes[node].info;
    const size_t per = static_cast<size_t>(li.h) * li.w * li.c;
    float*& stage = depth == 3 ? h->d_feat6 : h->d_feat;
    if (!stage) {
        void* p = nullptr;
        if ((rc = dev_alloc(h, static_cast<size_t>(h->max_batch) * per * 4, &p)) != RN_OK) return rc;
        stage = static_cast<float*>(p);
    }
    RN_HIP(hipMemcpyAsync(h->d_in_u8, bgr_nhwc, static_cast<size_t>(n) * h->im_side * h->im_side * 3, hipMemcpyHostToDevice, h->stream));
    if ((rc = features_device(h, h->d_in_u8, n, node, stage)) != RN_OK) return rc;
    RN_HIP(hipMemcpyAsync(feat, stage, static_cast<size_t>(n) * per * 4, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}
}  // namespace

extern "C" int rn_features_u8(rn_handle* h, const uint8_t* bgr_nhwc, int n, float* feat) { return features_host(h, 2, bgr_nhwc, n, feat); }

extern "C" int rn_features_depth_u8(rn_handle* h, int depth, const uint8_t* bgr_nhwc, int n, float* feat) {
    return features_host(h, depth, bgr_nhwc, n, feat);
}

// ---- two-slot host pipeline: the upload of batch k+1 overlaps the forward pass of batch k
extern "C" int rn_submit_u8(rn_handle* h, const uint8_t* bgr, int n, int slot) {
    if (!h || !bgr || slot < 0 || slot > 1) {
        rn_set_error("rn_submit_u8: bad argument");
        return RN_E_INVALID;
    }
    if (n < 1 || n > h->max_batch) {
        rn_set_error("rn_submit_u8: n = %d out of range (1..%d)", n, h->max_batch);
        return RN_E_RANGE;
    }
    rn_handle::HostSlot& sl = h->slots[slot];
    if (sl.busy) {
        rn_set_error("rn_submit_u8: slot %d holds results that were not collected", slot);
        return RN_E_STATE;
    }
    DeviceGuard guard(h->device);
    if (!h->copy_stream) RN_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!sl.d_in) {
        const size_t in_bytes = static_cast<size_t>(h->max_batch) * h->im_side * h->im_side * 3;
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&sl.d_in), in_bytes));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&sl.d_probs), static_cast<size_t>(h->max_batch) * h->num_classes * 4));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&sl.d_ids), static_cast<size_t>(h->max_batch) * 8));
        RN_HIP(hipHostMalloc(reinterpret_cast<void**>(&sl.h_probs), static_cast<size_t>(h->max_batch) * h->num_classes * 4, 0));
        RN_HIP(hipHostMalloc(reinterpret_cast<void**>(&sl.h_ids), static_cast<size_t>(h->max_batch) * 8, 0));
        RN_HIP(hipEventCreateWithFlags(&sl.uploaded, hipEventDisableTiming));
        RN_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    const size_t in_bytes = static_cast<size_t>(n) * h->im_side * h->im_side * 3;
    // from pageable memory this call returns once the bytes are staged: the previous batch's kernels, enqueued earlier on
    // the compute stream, run meanwhile; from pinned memory it is asynchronous outright
    RN_HIP(hipMemcpyAsync(sl.d_in, bgr, in_bytes, hipMemcpyHostToDevice, h->copy_stream));
    RN_HIP(hipEventRecord(sl.uploaded, h->copy_stream));
    RN_HIP(hipStreamWaitEvent(h->stream, sl.uploaded, 0));
    int rc = rn_forward_u8_device(h, sl.d_in, n, sl.d_probs, sl.d_ids);
    if (rc != RN_OK) return rc;
    RN_HIP(hipMemcpyAsync(sl.h_probs, sl.d_probs, static_cast<size_t>(n) * h->num_classes * 4, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipMemcpyAsync(sl.h_ids, sl.d_ids, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipEventRecord(sl.done, h->stream));
    sl.n = n;
    sl.busy = true;
    return RN_OK;
}

extern "C" int rn_collect(rn_handle* h, int slot, float* probs, int64_t* ids) {
    if (!h || !probs || !ids || slot < 0 || slot > 1) {
        rn_set_error("rn_collect: bad argument");
        return RN_E_INVALID;
    }
    rn_handle::HostSlot& sl = h->slots[slot];
    if (!sl.busy) {
        rn_set_error("rn_collect: nothing was submitted to slot %d", slot);
        return RN_E_STATE;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipEventSynchronize(sl.done));
    std::memcpy(probs, sl.h_probs, static_cast<size_t>(sl.n) * h->num_classes * 4);
    std::memcpy(ids, sl.h_ids, static_cast<size_t>(sl.n) * 8);
    sl.busy = false;
    return RN_OK;
}

// ---- caller-side image pipeline on the device (network.py:137-156)
// network.py:137-146: the centred square window of an h x w image (abs((w - h) // 2) with Python floor division)
void rn_center_crop_window(int hh, int ww, int* x0, int* y0, int* side) {
    if (hh == ww) {
        *x0 = *y0 = 0;
        *side = hh;
    } else if (ww > hh) {
        *x0 = (ww - hh) / 2;
        *y0 = 0;
        *side = hh;
    } else {
        // abs((w - h) // 2): floor division of a negative number rounds away from zero before abs()
        *x0 = 0;
        *y0 = (hh - ww + 1) / 2;
        *side = ww;
    }
}
// ... of a packed BGR image at `src`
rn_window rn_center_window(const uint8_t* src, int hh, int ww) {
    int x0, y0, side;
    rn_center_crop_window(hh, ww, &x0, &y0, &side);
    return {src + (static_cast<int64_t>(y0) * ww + x0) * 3, side, static_cast<int64_t>(ww) * 3};
}

extern "C" int rn_crop_resize_u8_device(rn_handle* h, const uint8_t* d_src, int src_h, int src_w, uint8_t* d_dst_batch,
                                        int index) {
    if (!h || !d_src || !d_dst_batch || src_h < 1 || src_w < 1 || index < 0 || index >= h->max_batch) {
        rn_set_error("rn_crop_resize_u8_device: bad argument (image %dx%d, slot %d of %d)", src_w, src_h, index,
                     h ? h->max_batch : 0);
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    const rn_window w = rn_center_window(d_src, src_h, src_w);
    const int S = h->im_side;
    return rn_launch_resize_u8(h->stream, w.src, w.side, w.side, w.row_bytes, d_dst_batch + static_cast<int64_t>(index) * S * S * 3, S, S);
}

int rn_check_batch(const char* who, const rn_handle* h, const void* ptr, int n) {
    if (!h || !ptr) {
        rn_set_error("%s: null argument", who);
        return RN_E_INVALID;
    }
    if (n < 1 || n > h->max_batch) {
        rn_set_error("%s: %d images out of range (1..%d)", who, n, h->max_batch);
        return RN_E_RANGE;
    }
    return RN_OK;
}

int rn_enqueue_resize_batch(rn_handle* h, int n, uint8_t* d_dst_batch, const std::function<rn_window(int)>& window) {
    int rc, set;
    if (!h->items_turn.done[0]) {      // the first use: two sets of max_batch entries (a failure here leaves what rn_destroy frees)
        for (auto& t : h->items)
            if (!t.cap && (rc = t.alloc(static_cast<size_t>(h->max_batch))) != RN_OK) return rc;
        if ((rc = h->items_turn.create()) != RN_OK) return rc;
    }
    if ((rc = h->items_turn.acquire(&set)) != RN_OK) return rc;
    const rn_table<rn_resize_item>& t = h->items[set];
    for (int i = 0; i < n; ++i) {
        const rn_window w = window(i);
        rn_resize_item_fill(&t.host[i], w.src, w.side, w.side, w.row_bytes, h->im_side);
    }
    if ((rc = t.upload(static_cast<size_t>(n), h->stream)) != RN_OK) return rc;
    if ((rc = rn_launch_resize_batch_u8(h->stream, t.dev, n, d_dst_batch, h->im_side)) != RN_OK) return rc;
    return h->items_turn.retire(h->stream);
}

extern "C" int rn_crop_resize_batch_u8_device(rn_handle* h, const uint8_t* const* d_srcs, const int* heights, const int* widths, int n,
                                              uint8_t* d_dst_batch) {
    if (!h || !d_srcs || !heights || !widths || !d_dst_batch || n < 1 || n > h->max_batch) {
        rn_set_error("rn_crop_resize_batch_u8_device: bad argument (%d images, max_batch %d)", n, h ? h->max_batch : 0);
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i)
        if (!d_srcs[i] || heights[i] < 1 || widths[i] < 1) {
            rn_set_error("rn_crop_resize_batch_u8_device: image %d is empty", i);
            return RN_E_INVALID;
        }
    DeviceGuard guard(h->device);
    return rn_enqueue_resize_batch(h, n, d_dst_batch, [&](int i) { return rn_center_window(d_srcs[i], heights[i], widths[i]); });
}

extern "C" int rn_classify_images_u8(rn_handle* h, const uint8_t* const* images, const int* heights, const int* widths, int n,
                                     float* probs, int64_t* ids) {
    int rc = check_call(h, n, images, probs, ids);
    if (rc != RN_OK) return rc;
    if (!heights || !widths) {
        rn_set_error("rn_classify_images_u8: heights / widths missing");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    // one staging buffer for the raw images, grown to the batch's total size: uploads and the resize launch are queued
    // on the handle's stream back to back
    // (only the centred square window of each image crosses PCIe: a 1920x1080 frame uploads 1080x1080)
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!images[i] || heights[i] < 1 || widths[i] < 1) {
            rn_set_error("rn_classify_images_u8: image %d is empty", i);
            return RN_E_INVALID;
        }
        const size_t side = static_cast<size_t>(heights[i] < widths[i] ? heights[i] : widths[i]);
        total += side * side * 3;
    }
    if ((rc = rn_grow_scratch(h, &h->d_raw, &h->raw_cap, total, "image staging")) != RN_OK) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const rn_window w = rn_center_window(images[i], heights[i], widths[i]);
        const size_t row = static_cast<size_t>(w.side) * 3;
        if (w.side == widths[i])
            RN_HIP(hipMemcpyAsync(h->d_raw + off, w.src, row * w.side, hipMemcpyHostToDevice, h->stream));
        else
            RN_HIP(hipMemcpy2DAsync(h->d_raw + off, row, w.src, static_cast<size_t>(w.row_bytes), row, w.side, hipMemcpyHostToDevice, h->stream));
        off += row * w.side;
    }
    // ONE resize launch for the batch (the packed windows' table goes up behind the images)
    off = 0;
    rc = rn_enqueue_resize_batch(h, n, h->d_in_u8, [&](int i) {
        const int side = heights[i] < widths[i] ? heights[i] : widths[i];
        const rn_window w = {h->d_raw + off, side, static_cast<int64_t>(side) * 3};
        off += static_cast<size_t>(side) * side * 3;
        return w;
    });
    if (rc != RN_OK) return rc;
    if ((rc = rn_forward_u8_device(h, h->d_in_u8, n, h->d_probs, h->d_ids)) != RN_OK) return rc;
    return rn_results_to_host(h, n, probs, ids);
}

extern "C" int rn_forward_f32(rn_handle* h, const float* rgb, int n, float* probs, int64_t* ids) {
    int rc = check_call(h, n, rgb, probs, ids);
    if (rc != RN_OK) return rc;
    if (fused_mode(h)) {
        rn_set_error("rn_forward_f32: 16-bit handles take uint8 input (use rn_forward_u8)");
        return RN_E_STATE;
    }
    DeviceGuard guard(h->device);
    float* in_node = static_cast<float*>(h->nodes[h->node_input].ptr);
    const size_t in_bytes = static_cast<size_t>(n) * h->im_side * h->im_side * 3 * 4;
    RN_HIP(hipMemcpyAsync(in_node, rgb, in_bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = rn_forward_f32_device(h, in_node, n, h->d_probs, h->d_ids)) != RN_OK) return rc;
    return rn_results_to_host(h, n, probs, ids);
}

extern "C" int rn_node_count(const rn_handle* h) { return h ? static_cast<int>(h->nodes.size()) : 0; }

extern "C" int rn_node_info_get(const rn_handle* h, int node_id, rn_node_info* out) {
    if (!h || !out || node_id < 0 || node_id >= static_cast<int>(h->nodes.size())) {
        rn_set_error("rn_node_info_get: bad argument");
        return RN_E_RANGE;
    }
    *out = h->nodes[node_id].info;
    return RN_OK;
}

extern "C" int rn_tap(rn_handle* h, int node_id, float* out, size_t cap_elems, size_t* n_elems) {
    if (!h || !out || node_id < 0 || node_id >= static_cast<int>(h->nodes.size())) {
        rn_set_error("rn_tap: bad argument");
        return RN_E_RANGE;
    }
    if (h->last_n < 1) {
        rn_set_error("rn_tap: no forward pass has run on this handle");
        return RN_E_STATE;
    }
    const NodeBuf& nb = h->nodes[node_id];
    if (!nb.ptr) {
        rn_set_error("rn_tap: node %s is not materialised on this handle (create with RN_FLAG_TAPS)", nb.info.name);
        return RN_E_STATE;
    }
    if (fused_mode(h)) {
        bool fused_away = false;
        for (size_t i = 0; i < h->stages.size(); ++i)
            fused_away |= node_id == h->stages[i].node_bn && rn_fused_stage_elided(h, static_cast<int>(i));
        if (fused_away) {
            rn_set_error("rn_tap: node %s is fused into its successor's kernel on this handle and never written "
                         "(create with RN_FLAG_STAGE_LAUNCHES)", nb.info.name);
            return RN_E_STATE;
        }
    }
    const bool shared_scratch = !(h->flags & RN_FLAG_TAPS) && !fused_mode(h);
    if (shared_scratch) {
        // a residual stage that runs as ONE matrix-core launch (rn_stage_f32m.hip) writes its output node (sK.bn2) only: the
        // first BN output never leaves the kernel
        for (size_t i = 0; i < h->stages.size(); ++i) {
            const StagePlan& s = h->stages[i];
            if (node_id == s.node_bn && s.node_bn2 >= 0 && rn_f32m_covers(h, static_cast<int>(i))) {
                rn_set_error("rn_tap: node %s stays inside the stage's matrix-core launch on this handle and is never written "
                             "(create with RN_FLAG_TAPS)", nb.info.name);
                return RN_E_STATE;
            }
        }
        const char* nm = nb.info.name;
        const size_t len = std::strlen(nm);
        const bool inter = (len > 5 && (!std::strcmp(nm + len - 5, ".conv") || !std::strcmp(nm + len - 5, ".pool"))) ||
                           (len > 4 && !std::strcmp(nm + len - 4, ".add"));
        if (inter) {
            rn_set_error("rn_tap: node %s shares scratch memory on this handle (create with RN_FLAG_TAPS)", nm);
            return RN_E_STATE;
        }
    }
    const size_t total = static_cast<size_t>(h->last_n) * node_elems(nb);
    if (n_elems) *n_elems = total;
    if (cap_elems < total) {
        rn_set_error("rn_tap: buffer too small (%zu < %zu elements)", cap_elems, total);
        return RN_E_RANGE;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipStreamSynchronize(h->stream));
    if (nb.dtype == RN_DTYPE_F32) {
        RN_HIP(hipMemcpy(out, nb.ptr, total * 4, hipMemcpyDeviceToHost));
    } else {
        float* tmp = nullptr;
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), total * 4));
        int rc = rn_launch_convert_to_f32(h->stream, nb.ptr, nb.dtype, tmp, static_cast<int64_t>(total));
        if (rc == RN_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = RN_E_HIP;
        if (rc == RN_OK && hipMemcpy(out, tmp, total * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = RN_E_HIP;
        (void)hipFree(tmp);
        if (rc != RN_OK) {
            if (rc == RN_E_HIP) rn_set_error("rn_tap: device copy failed");
            return rc;
        }
    }
    // a handle may store this tensor with its channels relabelled (frozen-channel folding, rn_fused_prepare): hand it out in the
    // reference's channel order
    {
        auto it = h->node_perm.find(node_id);
        if (it != h->node_perm.end()) {
            const int* perm = it->second.data();
            const int c = nb.info.c;
            std::vector<float> px(static_cast<size_t>(c));
            for (size_t q = 0; q < total / static_cast<size_t>(c); ++q) {
                float* pix = out + q * c;
                for (int p = 0; p < c; ++p) px[perm[p]] = pix[p];
                std::memcpy(pix, px.data(), static_cast<size_t>(c) * 4);
            }
        }
    }
    return RN_OK;
}

extern "C" int rn_set_profiling(rn_handle* h, int enable) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    h->profiling = enable != 0;
    h->timing_valid = false;
    return RN_OK;
}

extern "C" int rn_timing(rn_handle* h, rn_stage_ms* out) {
    if (!h || !out) {
        rn_set_error("rn_timing: bad argument");
        return RN_E_INVALID;
    }
    if (!h->timing_valid) {
        rn_set_error("rn_timing: no profiled forward pass (call rn_set_profiling(h,1) first)");
        return RN_E_STATE;
    }
    DeviceGuard guard(h->device);
    const int ns = static_cast<int>(h->stages.size());
    RN_HIP(hipEventSynchronize(h->events[2 + ns]));
    std::memset(out, 0, sizeof(*out));
    out->n_stages = ns;
    RN_HIP(hipEventElapsedTime(&out->preprocess_ms, h->events[0], h->events[1]));
    for (int i = 0; i < ns; ++i) RN_HIP(hipEventElapsedTime(&out->stage_ms[i], h->events[1 + i], h->events[2 + i]));
    RN_HIP(hipEventElapsedTime(&out->head_ms, h->events[1 + ns], h->events[2 + ns]));
    RN_HIP(hipEventElapsedTime(&out->total_ms, h->events[0], h->events[2 + ns]));
    return RN_OK;
}

extern "C" int rn_dominant_stage(const rn_handle* h) {
    if (!h) return -1;
    int best = 0;
    double bestf = -1;
    for (size_t i = 0; i < h->stages.size(); ++i) {
        const StagePlan& s = h->stages[i];
        const double f = 2.0 * s.conv_side * s.conv_side * 9.0 * s.cin * s.cout;
        if (f > bestf) {
            bestf = f;
            best = static_cast<int>(i);
        }
    }
    return best;
}

extern "C" int rn_stage_launch(const rn_handle* h, int stage) {
    if (!h || stage < 0 || stage >= static_cast<int>(h->stages.size())) {
        rn_set_error("rn_stage_launch: bad argument");
        return RN_E_RANGE;
    }
    return fused_mode(h) ? rn_fused_launch_rep(h, stage) : stage;
}

extern "C" int rn_device_malloc(rn_handle* h, size_t bytes, void** d_ptr) {
    if (!h || !d_ptr) {
        rn_set_error("rn_device_malloc: bad argument");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 16);
    if (e != hipSuccess) {
        rn_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return RN_E_NOMEM;
    }
    return RN_OK;
}

extern "C" int rn_device_free(rn_handle* h, void* d_ptr) {
    if (!h) {
        rn_set_error("null handle");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipFree(d_ptr));
    return RN_OK;
}

extern "C" int rn_memcpy_h2d(rn_handle* h, void* d_dst, const void* src, size_t bytes) {
    if (!h || !d_dst || !src) {
        rn_set_error("rn_memcpy_h2d: bad argument");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

extern "C" int rn_memcpy_d2h(rn_handle* h, void* dst, const void* d_src, size_t bytes) {
    if (!h || !dst || !d_src) {
        rn_set_error("rn_memcpy_d2h: bad argument");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

// ---- pinned host memory: what makes the host-buffer entries asynchronous (rn_submit_u8, rn_group_forward_u8)
extern "C" int rn_host_alloc(size_t bytes, void** ptr) {
    if (!ptr || bytes == 0) {
        rn_set_error("rn_host_alloc: bad argument");
        return RN_E_INVALID;
    }
    *ptr = nullptr;
    // portable: usable as a copy source for every device of the process (a group's shards come out of one buffer)
    hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        rn_set_error("rn_host_alloc: hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        (void)hipGetLastError();       // reported: it must not surface again as the next kernel's "launch failure"
        *ptr = nullptr;
        return RN_E_NOMEM;
    }
    return RN_OK;
}

extern "C" int rn_host_free(void* ptr) {
    if (!ptr) return RN_OK;
    RN_HIP(hipHostFree(ptr));
    return RN_OK;
}

extern "C" int rn_const_info(const rn_handle* h, int info[4]) {
    if (!h || !info) {
        rn_set_error("rn_const_info: bad argument");
        return RN_E_INVALID;
    }
    info[0] = -1;
    info[1] = info[2] = info[3] = 0;
    if (fused_mode(h)) rn_fused_const_info(h, info);
    return RN_OK;
}

extern "C" int rn_frozen_info(const rn_handle* h, int info[4]) {
    if (!h || !info) {
        rn_set_error("rn_frozen_info: bad argument");
        return RN_E_INVALID;
    }
    fused_mode(h) ? rn_fused_frozen_info(h, info) : rn_f32m_frozen_info(h, info);
    return RN_OK;
}
