// Huffman stage of the baseline-JPEG decode on the GPU (the decode step is rn_jpeg_huff.h, its host model
// rn_jpeg_huff_model.h): the scan bytes of a batch of files in, int16 quantised coefficients out, in the layout jpeg_idct_kernel
// reads, byte for byte what rn_jpeg_entropy_decode writes.  Integer arithmetic, no floating point, no atomics on results.
//   huff_sync_kernel   one lane per subsequence of RN_JPEG_SUBSEQ_BYTES raw bytes, 256 per workgroup, the image's tables in LDS:
//                      decodes from the guessed state, then again from the left neighbour's exit state (kept in LDS) in
//                      __syncthreads rounds until a round changes nothing -- at most 255 rounds, the group's size.
//   huff_cross_kernel  ONE workgroup per image: a walker per group decodes from the last state of the group in front until it meets
//                      what is stored, in rounds, at most as many as the image has groups; then the exclusive scan of the
//                      subsequences' block counts.
//   huff_write_kernel  one lane per subsequence decodes from its entry state with the coefficient writer and checks that its exit
//                      state is the stored one: a chain that is consistent from subsequence 0 is the sequential decode.
//   huff_dc_kernel     one workgroup per component: the DC differences summed in scan order, predictor reset at restart
//                      intervals, the host pass's two limit checks.
// All four are ONE launch per batch (blockIdx.z or blockIdx.x = image, a device table of per-image descriptors).  Every loop is
// bounded by a length the host computed; no lane waits for another workgroup; the order between workgroups is the launches'.
// Reads stay inside [scan, scan + scan_len), writes inside the image's block grids, whatever the bytes are.
#include "rn_jpeg_dev.h"
#include "rn_jpeg_huff_model.h"

#include <algorithm>

using namespace rn_jpeg_huff;

namespace {

__device__ __forceinline__ void load_tables(Tables* s_t, const Tables* g) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(g);
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_t);
    for (uint32_t k = threadIdx.x; k < sizeof(Tables) / 4; k += blockDim.x) dst[k] = src[k];
    __syncthreads();
}

__global__ __launch_bounds__(256) void huff_sync_kernel(const HuffDev* __restrict__ descs, int32_t* rounds) {
    const HuffDev& d = descs[blockIdx.z];
    const uint32_t first = blockIdx.x * kGroup;
    if (first >= d.nsub) return;                   // (uniform per workgroup: in front of every barrier)
    __shared__ Tables s_t;
    __shared__ State s_exit[kGroup];
    load_tables(&s_t, d.tables);
    const Ctx c{d.scan, d.scan_len, &s_t, d.g};
    const uint32_t t = threadIdx.x, i = first + t;
    const bool live = i < d.nsub;
    const uint32_t end = live ? subseq_end_bit(d.scan_len, RN_JPEG_SUBSEQ_BYTES, i) : 0;
    NoSink none;
    State mine{0, kInvalid, 0, 0};
    if (live) mine = decode_subsequence(c, guess(d.scan, d.scan_len, RN_JPEG_SUBSEQ_BYTES, i), end, none);
    s_exit[t] = mine;
    __syncthreads();
    const uint32_t count = min(static_cast<uint32_t>(kGroup), d.nsub - first);
    State last_in{0, kInvalid, 0, 0};
    bool have_last = false;
    int taken = 0;
    for (uint32_t round = 1; round < count; ++round) {
        bool changed = false;
        State out = mine;
        if (live && t > 0) {
            const State in = entry_of(s_exit[t - 1]);
            if (!have_last || in.p != last_in.p || in.sk != last_in.sk) {
                out = decode_subsequence(c, in, end, none);
                last_in = in;
                have_last = true;
                changed = !same(out, mine);
            }
        }
        __syncthreads();                           // every lane has read its neighbour's state
        if (changed) s_exit[t] = mine = out;
        if (!__syncthreads_or(changed)) break;
        taken = static_cast<int>(round);
    }
    if (live) d.exit_state[i] = mine;
    if (t == 0) atomicMax(&rounds[2 * blockIdx.z], taken);
}

__global__ __launch_bounds__(256) void huff_cross_kernel(const HuffDev* __restrict__ descs, int32_t* rounds) {
    const HuffDev& d = descs[blockIdx.x];
    if (d.nsub == 0) return;
    __shared__ Tables s_t;
    __shared__ uint32_t s_scan[256];
    load_tables(&s_t, d.tables);
    const Ctx c{d.scan, d.scan_len, &s_t, d.g};
    const uint32_t t = threadIdx.x, nsub = d.nsub;
    const uint32_t ngroups = (nsub + kGroup - 1) / kGroup;
    State* chain = d.exit_state;
    NoSink none;
    int taken = 0;
    for (uint32_t round = 1; round < ngroups; ++round) {
        bool changed = false;
        for (uint32_t g0 = 1; g0 < ngroups; g0 += 256) {
            const uint32_t g = g0 + t;
            const bool live = g < ngroups;
            State s{0, kInvalid, 0, 0};
            if (live) s = chain[g * kGroup - 1];
            __syncthreads();                       // every walker has read the state it starts from
            if (live) {
                const uint32_t stop = min(nsub, (g + 1) * kGroup);
                for (uint32_t j = g * kGroup; j < stop; ++j) {
                    const State out = decode_subsequence(c, entry_of(s), subseq_end_bit(d.scan_len, RN_JPEG_SUBSEQ_BYTES, j), none);
                    if (same(out, chain[j])) break;
                    chain[j] = out;
                    changed = true;
                    s = out;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(changed)) break;
        taken = static_cast<int>(round);
    }
    // exclusive scan of the block counts
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nsub; i0 += 256) {
        const uint32_t i = i0 + t;
        const uint32_t v = i < nsub ? chain[i].n : 0;
        s_scan[t] = v;
        __syncthreads();
        for (uint32_t o = 1; o < 256; o <<= 1) {
            const uint32_t a = t >= o ? s_scan[t - o] : 0;
            __syncthreads();
            s_scan[t] += a;
            __syncthreads();
        }
        if (i < nsub) d.base[i] = carry + s_scan[t] - v;
        carry += s_scan[255];
        __syncthreads();
    }
    if (t == 0) rounds[2 * blockIdx.x + 1] = taken;
}

__global__ __launch_bounds__(256) void huff_write_kernel(const HuffDev* __restrict__ descs, int32_t* status) {
    const HuffDev& d = descs[blockIdx.z];
    const uint32_t first = blockIdx.x * kGroup;
    if (first >= d.nsub) return;
    __shared__ Tables s_t;
    load_tables(&s_t, d.tables);
    const uint32_t i = first + threadIdx.x;
    if (i >= d.nsub) return;                       // (behind the only barrier)
    const Ctx c{d.scan, d.scan_len, &s_t, d.g};
    Writer w{&c.g, &s_t, {d.coef[0], d.coef[1], d.coef[2]}, d.base[i]};
    const State entry = i == 0 ? guess(d.scan, d.scan_len, RN_JPEG_SUBSEQ_BYTES, 0) : entry_of(d.exit_state[i - 1]);
    const int32_t st = write_lane(c, entry, d.exit_state[i], subseq_end_bit(d.scan_len, RN_JPEG_SUBSEQ_BYTES, i), i + 1 == d.nsub, w);
    if (st != RN_JPEG_ST_OK) atomicMax(&status[blockIdx.z], st);
}

__global__ __launch_bounds__(256) void huff_dc_kernel(const HuffDev* __restrict__ descs, int32_t* status) {
    const HuffDev& d = descs[blockIdx.z];
    const int comp = blockIdx.x;
    if (d.nsub == 0 || comp >= d.g.ncomp) return;
    __shared__ long long s_tail[256], s_in[256];
    __shared__ int s_reset[256];
    const uint32_t t = threadIdx.x, nb = static_cast<uint32_t>(d.nblk[comp]);
    const uint32_t per = (nb + 255) / 256, j0 = min(t * per, nb), j1 = min(j0 + per, nb);
    bool reset = false;
    s_tail[t] = dc_run(d.g, comp, j0, j1, 0, d.q0[comp], d.coef[comp], nullptr, &reset);
    s_reset[t] = reset;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < 256; ++k) {
            s_in[k] = run;
            run = s_reset[k] ? s_tail[k] : run + s_tail[k];
        }
    }
    __syncthreads();
    int32_t st = RN_JPEG_ST_OK;
    dc_run(d.g, comp, j0, j1, s_in[t], d.q0[comp], d.coef[comp], &st, nullptr);
    if (st != RN_JPEG_ST_OK) atomicMax(&status[blockIdx.z], st);
}

int huff_state(rn_handle* h, JpegState** out) {
    int rc = rn_jpeg_state(h, out);
    if (rc != RN_OK) return rc;
    JpegState* s = *out;
    if (!s->scan_done) {                           // the first Huffman call on this handle
        const size_t mb = static_cast<size_t>(h->max_batch);
        for (int k = 0; k < 2; ++k) {
            if (!s->huff[k].cap && (rc = s->huff[k].alloc(mb)) != RN_OK) return rc;
            if (!s->huff_tables[k].cap && (rc = s->huff_tables[k].alloc(mb)) != RN_OK) return rc;
            if (!s->huff_status[k].cap && (rc = s->huff_status[k].alloc(mb)) != RN_OK) return rc;
            if (!s->huff_rounds[k].cap && (rc = s->huff_rounds[k].alloc(2 * mb)) != RN_OK) return rc;
        }
        if (!s->huff_timer.t0 && (rc = s->huff_timer.create()) != RN_OK) return rc;
        RN_HIP(hipEventCreateWithFlags(&s->scan_done, hipEventDisableTiming));
        s->huff_ready = true;
    }
    return RN_OK;
}

int check_files(const char* who, rn_handle* h, const rn_jpeg_file* files, int n, const void* status) {
    const int rc = rn_check_batch(who, h, files, n);
    if (rc != RN_OK) return rc;
    if (!status) {
        rn_set_error("%s: null argument", who);
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i)
        if (!files[i].bytes || !rn_jpeg_info_ok(files[i].info)) {
            rn_set_error("%s: file %d is not a supported JPEG as rn_jpeg_probe[_oriented] describes one (%dx%d, %d components, sampling %dx%d, supported %d)",
                         who, i, files[i].info.width, files[i].info.height, files[i].info.ncomp, files[i].info.hsamp,
                         files[i].info.vsamp, files[i].info.supported);
            return RN_E_INVALID;
        }
    return RN_OK;
}

// Upload + the launches of the four phases for n checked files.  d_coeffs == nullptr: into the handle's coefficient scratch, image i
// at offsets[i] (int16 elements).  The statuses and round counts arrive in the host side of set *set's tables behind the launches.
int enqueue_huffman(rn_handle* h, JpegState* st, const rn_jpeg_file* files, int n, int16_t* const* d_coeffs, int* set_out,
                    std::vector<size_t>* offsets) {
    size_t scan_total = 0, sub_total = 0, coef_total = 0;
    uint32_t max_groups = 0;
    std::vector<int32_t> pre(static_cast<size_t>(n));
    std::vector<uint32_t> nsubs(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        pre[i] = precheck(files[i].scan.scan_len);
        nsubs[i] = pre[i] == RN_JPEG_ST_OK ? subseq_count(static_cast<uint32_t>(files[i].scan.scan_len), RN_JPEG_SUBSEQ_BYTES) : 0;
        if (nsubs[i]) scan_total += (static_cast<size_t>(files[i].scan.scan_len) + 15) & ~static_cast<size_t>(15);
        sub_total += nsubs[i];
        max_groups = std::max(max_groups, (nsubs[i] + kGroup - 1) / kGroup);
        coef_total += rn_jpeg::coeff_count(files[i].info);
    }
    int rc, set;
    if ((rc = st->turn.acquire(&set)) != RN_OK) return rc;
    if ((rc = rn_grow_scratch(h, &st->d_scan, &st->scan_cap, scan_total, "JPEG scan bytes")) != RN_OK) return rc;
    if ((rc = rn_grow_scratch(h, &st->d_chain, &st->chain_cap, sub_total * (sizeof(State) + sizeof(uint32_t)), "JPEG decoder states")) != RN_OK)
        return rc;
    if (!d_coeffs && (rc = rn_grow_scratch(h, &st->d_coef, &st->coef_cap, coef_total, "JPEG coefficients")) != RN_OK) return rc;
    const rn_table<HuffDev>& tab = st->huff[set];
    // the previous call's launches read the scan scratch: the copy stream starts behind them
    RN_HIP(hipStreamWaitEvent(h->copy_stream, st->scan_done, 0));
    State* states = reinterpret_cast<State*>(st->d_chain);
    uint32_t* bases = reinterpret_cast<uint32_t*>(st->d_chain + sub_total * sizeof(State));
    size_t scan_off = 0, sub_off = 0, coef_off = 0;
    if (offsets) offsets->assign(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; ++i) {
        const rn_jpeg_info& f = files[i].info;
        HuffDev& d = tab.host[i];
        std::memset(&d, 0, sizeof(d));
        fill_tables(files[i].scan, f, &st->huff_tables[set].host[i]);
        d.tables = st->huff_tables[set].dev + i;
        d.g = geometry(f);
        d.nsub = nsubs[i];
        d.scan_len = nsubs[i] ? static_cast<uint32_t>(files[i].scan.scan_len) : 0;
        d.scan = st->d_scan + scan_off;
        d.exit_state = states + sub_off;
        d.base = bases + sub_off;
        int16_t* coef = d_coeffs ? d_coeffs[i] : st->d_coef + coef_off;
        if (offsets) (*offsets)[i] = coef_off;
        size_t count = 0;
        for (int c = 0; c < f.ncomp; ++c) {
            d.coef[c] = coef + count;
            d.nblk[c] = f.blocks_w[c] * f.blocks_h[c];
            d.q0[c] = f.qt[c][0];
            count += static_cast<size_t>(d.nblk[c]) * 64;
        }
        coef_off += count;
        if (nsubs[i]) {
            RN_HIP(hipMemcpyAsync(st->d_scan + scan_off, files[i].bytes, d.scan_len, hipMemcpyHostToDevice, h->copy_stream));
            scan_off += (static_cast<size_t>(d.scan_len) + 15) & ~static_cast<size_t>(15);
        }
        sub_off += nsubs[i];
        st->huff_status[set].host[i] = pre[i];
        st->huff_rounds[set].host[2 * i] = st->huff_rounds[set].host[2 * i + 1] = 0;
    }
    RN_HIP(hipEventRecord(st->uploaded, h->copy_stream));
    const size_t un = static_cast<size_t>(n);
    if ((rc = tab.upload(un, h->stream)) != RN_OK || (rc = st->huff_tables[set].upload(un, h->stream)) != RN_OK ||
        (rc = st->huff_status[set].upload(un, h->stream)) != RN_OK || (rc = st->huff_rounds[set].upload(2 * un, h->stream)) != RN_OK)
        return rc;
    RN_HIP(hipStreamWaitEvent(h->stream, st->uploaded, 0));
    if ((rc = st->huff_timer.start(h->stream)) != RN_OK) return rc;
    // EOB leaves zeros: the coefficients start as zeros
    if (!d_coeffs) {
        RN_HIP(hipMemsetAsync(st->d_coef, 0, coef_total * sizeof(int16_t), h->stream));
    } else {
        for (int i = 0; i < n; ++i)
            RN_HIP(hipMemsetAsync(d_coeffs[i], 0, rn_jpeg::coeff_count(files[i].info) * sizeof(int16_t), h->stream));
    }
    if (max_groups) {
        (void)hipGetLastError();
        int32_t* d_status = st->huff_status[set].dev;
        int32_t* d_rounds = st->huff_rounds[set].dev;
        hipLaunchKernelGGL(huff_sync_kernel, dim3(max_groups, 1, n), dim3(256), 0, h->stream, tab.dev, d_rounds);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(huff_cross_kernel, dim3(n), dim3(256), 0, h->stream, tab.dev, d_rounds);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(huff_write_kernel, dim3(max_groups, 1, n), dim3(256), 0, h->stream, tab.dev, d_status);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(huff_dc_kernel, dim3(3, 1, n), dim3(256), 0, h->stream, tab.dev, d_status);
        RN_CHECK_LAUNCH();
    }
    if ((rc = st->huff_timer.stop(h->stream)) != RN_OK) return rc;
    RN_HIP(hipEventRecord(st->scan_done, h->stream));
    RN_HIP(hipMemcpyAsync(st->huff_status[set].host, st->huff_status[set].dev, un * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipMemcpyAsync(st->huff_rounds[set].host, st->huff_rounds[set].dev, 2 * un * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    st->last_set = set;
    *set_out = set;
    return st->turn.retire(h->stream);
}

}  // namespace

extern "C" int rn_jpeg_scan_probe(const uint8_t* data, size_t len, rn_jpeg_scan* out) {
    if (!data || !out) {
        rn_set_error("rn_jpeg_scan_probe: null argument");
        return RN_E_INVALID;
    }
    const int rc = scan_probe(data, len, out);
    if (rc != RN_OK) rn_set_error("rn_jpeg_scan_probe: not a JPEG file, or its headers are truncated");
    return rc;
}

extern "C" int rn_jpeg_scan_probe_oriented(const uint8_t* data, size_t len, rn_jpeg_scan* out) {
    if (!data || !out) {
        rn_set_error("rn_jpeg_scan_probe_oriented: null argument");
        return RN_E_INVALID;
    }
    const int rc = scan_probe(data, len, out, true);
    if (rc != RN_OK) rn_set_error("rn_jpeg_scan_probe_oriented: not a JPEG file, or its headers are truncated");
    return rc;
}

extern "C" int rn_jpeg_huffman_model(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap,
                                     int subseq_bytes, int32_t* status) {
    const char* why = "";
    const int rc = model(data, len, info, coeffs, cap, subseq_bytes, status, nullptr, &why);
    if (rc != RN_OK) rn_set_error("rn_jpeg_huffman_model: %s", why);
    return rc;
}

extern "C" int rn_jpeg_huffman_batch_device(rn_handle* h, const rn_jpeg_file* files, int n, int16_t* const* d_coeffs, int32_t* status) {
    int rc = check_files("rn_jpeg_huffman_batch_device", h, files, n, status);
    if (rc != RN_OK) return rc;
    if (d_coeffs)
        for (int i = 0; i < n; ++i)
            if (!d_coeffs[i]) {
                rn_set_error("rn_jpeg_huffman_batch_device: image %d has no destination", i);
                return RN_E_INVALID;
            }
    DeviceGuard guard(h->device);
    JpegState* st = nullptr;
    int set = 0;
    if ((rc = huff_state(h, &st)) != RN_OK) return rc;
    if ((rc = enqueue_huffman(h, st, files, n, d_coeffs, &set, nullptr)) != RN_OK) return rc;
    RN_HIP(hipStreamSynchronize(h->stream));
    std::memcpy(status, st->huff_status[set].host, static_cast<size_t>(n) * sizeof(int32_t));
    return RN_OK;
}

extern "C" int rn_jpeg_huffman_batch(rn_handle* h, const rn_jpeg_file* files, int n, int16_t* const* coeffs_host, int32_t* status) {
    int rc = check_files("rn_jpeg_huffman_batch", h, files, n, status);
    if (rc != RN_OK) return rc;
    if (!coeffs_host) {
        rn_set_error("rn_jpeg_huffman_batch: null argument");
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i)
        if (!coeffs_host[i]) {
            rn_set_error("rn_jpeg_huffman_batch: image %d has no destination", i);
            return RN_E_INVALID;
        }
    DeviceGuard guard(h->device);
    JpegState* st = nullptr;
    int set = 0;
    std::vector<size_t> offsets;
    if ((rc = huff_state(h, &st)) != RN_OK) return rc;
    if ((rc = enqueue_huffman(h, st, files, n, nullptr, &set, &offsets)) != RN_OK) return rc;
    RN_HIP(hipStreamSynchronize(h->stream));
    std::memcpy(status, st->huff_status[set].host, static_cast<size_t>(n) * sizeof(int32_t));
    for (int i = 0; i < n; ++i)
        if (status[i] == RN_JPEG_ST_OK)
            RN_HIP(hipMemcpyAsync(coeffs_host[i], st->d_coef + offsets[i], rn_jpeg::coeff_count(files[i].info) * sizeof(int16_t),
                                  hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

extern "C" int rn_classify_jpeg_files(rn_handle* h, const rn_jpeg_file* files, int n, float* probs, int64_t* ids, int32_t* status) {
    int rc = check_files("rn_classify_jpeg_files", h, files, n, status);
    if (rc != RN_OK) return rc;
    if (!probs || !ids) {
        rn_set_error("rn_classify_jpeg_files: null buffer");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    JpegState* st = nullptr;
    int set = 0;
    std::vector<size_t> offsets;
    if ((rc = huff_state(h, &st)) != RN_OK) return rc;
    if ((rc = enqueue_huffman(h, st, files, n, nullptr, &set, &offsets)) != RN_OK) return rc;
    std::vector<rn_jpeg_job> jobs(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) jobs[i] = rn_jpeg_job{&files[i].info, st->d_coef + offsets[i], true};
    if ((rc = rn_jpeg_classify_jobs(h, st, jobs.data(), n, probs, ids)) != RN_OK) return rc;      // (waits for the stream)
    std::memcpy(status, st->huff_status[set].host, static_cast<size_t>(n) * sizeof(int32_t));
    for (int i = 0; i < n; ++i)
        if (status[i] != RN_JPEG_ST_OK) {          // its pixels came from unspecified coefficients
            ids[i] = -1;
            std::memset(probs + static_cast<size_t>(i) * h->num_classes, 0, static_cast<size_t>(h->num_classes) * sizeof(float));
        }
    return RN_OK;
}

extern "C" int rn_jpeg_last_huffman_ms(rn_handle* h, float* ms) {
    const JpegState* st = h ? static_cast<const JpegState*>(h->jpeg) : nullptr;
    return rn_timer::read("rn_jpeg_last_huffman_ms", h, st && st->huff_ready ? &st->huff_timer : nullptr,
                          "no JPEG batch has been Huffman-decoded on this handle", h ? h->device : 0, ms);
}

extern "C" int rn_jpeg_last_huffman_rounds(rn_handle* h, int n, int32_t* inside, int32_t* across) {
    const JpegState* st = h ? static_cast<const JpegState*>(h->jpeg) : nullptr;
    if (!st || !st->huff_ready || !inside || !across || n < 1 || n > h->max_batch) {
        rn_set_error("rn_jpeg_last_huffman_rounds: no Huffman batch on this handle, a null pointer, or n out of range");
        return RN_E_INVALID;
    }
    DeviceGuard guard(h->device);
    RN_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        inside[i] = st->huff_rounds[st->last_set].host[2 * i];
        across[i] = st->huff_rounds[st->last_set].host[2 * i + 1];
    }
    return RN_OK;
}
