// The Huffman pass of the output JPEG on the GPU (the per-position encoder and the host model are
// rn_jpeg_huffenc.h): int16 quantised coefficients in device memory in, the bytes of the file's scan and EOI out.  Four phases,
// each ONE set of launches per batch (blockIdx.z = image, a device table of per-image descriptors); order between phases is the
// launches' order, and no workgroup waits for another inside a launch.
//   huffenc_lengths_kernel   a wave per block, a lane per zigzag position: the block's 128 bytes are read as 32 dwords and
//                            permuted into zigzag order, __ballot gives the non-zero mask, piece() a lane's bits, a wave sum the
//                            block's bit count; a refusal raises the image's status word (atomicMax).
//   sum_tiles / scan_sums / scan_tiles   the exclusive scan of the counts per image in scan order: sums of kScanTile counts, one
//                            workgroup per image scans the sums (carrying over as many rounds as the host computed) and stores
//                            the image's total, every tile is scanned from its sum.  In place: counts become bit offsets.
//   huffenc_scatter_kernel   a wave per block again: a wave prefix sum of the lanes' lengths gives every lane its offset, the
//                            block is assembled in LDS at its bit phase (at most 31 + 1658 + 7 bits: 53 words) and flushed with
//                            one word per lane -- inner words are stored, the first and the last merged with atomicOr into the
//                            zeroed stream, which commutes.  The last block appends the 1-bits that pad the last byte.
//   count_ff / scan_sums / huffenc_stuff_kernel   a dword of the unstuffed stream per lane, kStuffChunk bytes per workgroup: FF
//                            bytes per chunk, their scan (the image's FF total), then byte i goes to i + (FF bytes in front of it)
//                            with 00 behind every FF; the lane that holds the last byte appends FF D9.
// The host reads the n bit totals and statuses after the offsets and the n FF totals after the count, and sizes the two streams
// from them (rn_grow_scratch: a failure returns before anything more is enqueued).  No floating point; every loop's trip count
// is a constant or comes from the descriptor; every address comes from a block number checked against the image's block count
// or a byte number checked against its stream length.
#include "rn_internal.h"
#include "rn_jpeg_huffenc.h"

#include <algorithm>
#include <vector>

namespace {

using namespace rn_jpeg_huffenc;

constexpr int kWg = 256;
constexpr int kWaves = kWg / 64;
constexpr int kBlockWords = (31 + kMaxBlockBits + 7 + 31) / 32;      // 53
static_assert(kBlockWords <= 64, "a lane flushes one word");
static_assert(kScanTile == kWg && kStuffChunk == 4 * kWg, "an element per lane");

struct ImgOut {
    uint32_t total_bits;      // the scan's last element: the unstuffed bit total
    uint32_t total_ff;        // FF bytes of the unstuffed stream
    int32_t status;
    uint32_t pad;
};

struct HuffEncDev {
    const int16_t* coef[3];   // [blocks_h][blocks_w][64] per component
    uint32_t* bits;           // [nblocks] bit counts, then bit offsets, scan order
    uint32_t* sums;           // tile sums of phase 2, chunk counts of phase 4
    uint32_t* raw;            // the unstuffed stream, zeroed, raw_words dwords
    uint8_t* out;             // the stuffed stream and EOI, out_bytes bytes
    ImgOut* res;
    uint32_t mcus_x;
    uint32_t nblocks;         // 0: the image takes no part in this launch
    uint32_t nsums;           // tiles or chunks
    uint32_t rounds;          // ceil(nsums / kWg): the trips of scan_sums
    uint32_t total_bits, nbytes, raw_words;
    uint32_t out_bytes;       // nbytes + total_ff + 2
};

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// Exclusive prefix of v over the workgroup and the workgroup's sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t wg_exclusive(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const uint32_t inc = wave_inclusive(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t s = s_wave[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();                  // (s_wave is free for the next call)
    *total = all;
    return before + inc - v;
}

// Lane `lane` of the wave that holds block s (< d.nblocks): its piece.
__device__ __forceinline__ Piece lane_piece(const HuffEncDev& d, const Tables& t, uint32_t s, int lane) {
    const Where at = locate(d.mcus_x, s);
    const int16_t* comp = d.coef[at.comp];
    const uint32_t* blk = reinterpret_cast<const uint32_t*>(comp + at.block * 64);
    const uint32_t pair = lane < 32 ? blk[lane] : 0u;            // natural positions 2 lane, 2 lane + 1
    const int nat = t.natural[lane];
    const uint32_t w = __shfl(pair, nat >> 1, 64);
    int val = static_cast<int16_t>(nat & 1 ? w >> 16 : w & 0xFFFFu);
    const uint64_t mask = __ballot(val != 0);
    if (lane == 0 && at.pred >= 0) val -= comp[at.pred * 64];
    return piece(t, at.comp ? 1 : 0, lane, val, mask);
}

__global__ __launch_bounds__(kWg) void huffenc_lengths_kernel(const HuffEncDev* __restrict__ descs, const Tables* __restrict__ tables) {
    const HuffEncDev& d = descs[blockIdx.z];
    const int lane = threadIdx.x & 63;
    const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));      // (the wave's block: scalar)
    if (s >= d.nblocks) return;                                  // (uniform per wave; the kernel has no barrier)
    const Piece p = lane_piece(d, *tables, s, lane);
    const uint32_t total = __shfl(wave_inclusive(p.len), 63, 64);
    if (lane == 0) d.bits[s] = total;
    if (p.status != RN_JPEG_ENC_ST_OK) atomicMax(&d.res->status, p.status);
}

__global__ __launch_bounds__(kWg) void huffenc_sum_tiles_kernel(const HuffEncDev* __restrict__ descs) {
    const HuffEncDev& d = descs[blockIdx.z];
    if (blockIdx.x >= d.nsums || d.nblocks == 0) return;         // (uniform per workgroup: in front of every barrier)
    __shared__ uint32_t s_wave[kWaves];
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x;
    uint32_t total;
    wg_exclusive(i < d.nblocks ? d.bits[i] : 0u, s_wave, &total);
    if (threadIdx.x == 0) d.sums[blockIdx.x] = total;
}

// sums[0 .. nsums) -> their exclusive scan, and the image's total into res (phase 2: total_bits, phase 4: total_ff)
__global__ __launch_bounds__(kWg) void huffenc_scan_sums_kernel(const HuffEncDev* __restrict__ descs, int phase) {
    const HuffEncDev& d = descs[blockIdx.x];
    if (d.nblocks == 0) return;
    __shared__ uint32_t s_wave[kWaves];
    uint32_t carry = 0;
    for (uint32_t r = 0; r < d.rounds; ++r) {
        const uint32_t i = r * kWg + threadIdx.x;
        uint32_t total;
        const uint32_t before = wg_exclusive(i < d.nsums ? d.sums[i] : 0u, s_wave, &total);
        if (i < d.nsums) d.sums[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (phase == 2)
            d.res->total_bits = carry;
        else
            d.res->total_ff = carry;
    }
}

__global__ __launch_bounds__(kWg) void huffenc_scan_tiles_kernel(const HuffEncDev* __restrict__ descs) {
    const HuffEncDev& d = descs[blockIdx.z];
    if (blockIdx.x >= d.nsums || d.nblocks == 0) return;
    __shared__ uint32_t s_wave[kWaves];
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x;
    uint32_t total;
    const uint32_t before = wg_exclusive(i < d.nblocks ? d.bits[i] : 0u, s_wave, &total);
    if (i < d.nblocks) d.bits[i] = d.sums[blockIdx.x] + before;
}

__global__ __launch_bounds__(kWg) void huffenc_scatter_kernel(const HuffEncDev* __restrict__ descs, const Tables* __restrict__ tables) {
    const HuffEncDev& d = descs[blockIdx.z];
    if (blockIdx.x * kWaves >= d.nblocks) return;                // (uniform per workgroup: in front of every barrier)
    __shared__ uint32_t s_words[kWaves][kBlockWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave);      // (the wave's block: scalar)
    const bool live = s < d.nblocks;
    if (lane < kBlockWords) s_words[wave][lane] = 0;
    __syncthreads();
    uint32_t base = 0, nwords = 0;
    if (live) {
        const Piece p = lane_piece(d, *tables, s, lane);
        const uint32_t inc = wave_inclusive(p.len);
        const uint32_t total = __shfl(inc, 63, 64);
        base = d.bits[s];
        const uint32_t phase = base & 31u;
        uint32_t* words = s_words[wave];
        put_bits(phase + inc - p.len, p.v, p.len, [&](uint32_t w, uint32_t v) { atomicOr(words + w, v); });
        uint32_t pad = 0;
        if (s + 1 == d.nblocks) {                                // the last byte is padded with 1-bits
            pad = (8u - ((base + total) & 7u)) & 7u;
            if (lane == 0) put_bits(phase + total, (1u << pad) - 1u, pad, [&](uint32_t w, uint32_t v) { atomicOr(words + w, v); });
        }
        nwords = (phase + total + pad + 31u) >> 5;               // <= kBlockWords
    }
    __syncthreads();
    if (live && static_cast<uint32_t>(lane) < nwords) {
        const uint32_t at = (base >> 5) + lane;
        const uint32_t v = byte_swap(s_words[wave][lane]);
        if (at < d.raw_words) {
            if (lane == 0 || static_cast<uint32_t>(lane) + 1 == nwords) {
                if (v) atomicOr(d.raw + at, v);                  // shared with the neighbouring block
            } else {
                d.raw[at] = v;
            }
        }
    }
}

__global__ __launch_bounds__(kWg) void huffenc_count_ff_kernel(const HuffEncDev* __restrict__ descs) {
    const HuffEncDev& d = descs[blockIdx.z];
    if (blockIdx.x >= d.nsums || d.nblocks == 0) return;
    __shared__ uint32_t s_wave[kWaves];
    const uint32_t w = blockIdx.x * kWg + threadIdx.x;
    const bool in = 4ull * w < d.nbytes && w < d.raw_words;
    uint32_t total;
    wg_exclusive(in ? count_ff(d.raw[w], min(4u, d.nbytes - 4u * w)) : 0u, s_wave, &total);
    if (threadIdx.x == 0) d.sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kWg) void huffenc_stuff_kernel(const HuffEncDev* __restrict__ descs) {
    const HuffEncDev& d = descs[blockIdx.z];
    if (blockIdx.x >= d.nsums || d.nblocks == 0) return;
    __shared__ uint32_t s_wave[kWaves];
    const uint32_t w = blockIdx.x * kWg + threadIdx.x;
    const bool in = 4ull * w < d.nbytes && w < d.raw_words;
    const uint32_t valid = in ? min(4u, d.nbytes - 4u * w) : 0u;
    const uint32_t word = in ? d.raw[w] : 0u;
    const uint32_t ff = count_ff(word, valid);
    uint32_t total;
    uint32_t to = 4u * w + d.sums[blockIdx.x] + wg_exclusive(ff, s_wave, &total);
    if (!in) return;
    if (ff == 0 && valid == 4 && (to & 3u) == 0 && to + 4u <= d.out_bytes) {
        *reinterpret_cast<uint32_t*>(d.out + to) = word;
        to += 4;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (j < valid) {
                const uint32_t b = (word >> (8 * j)) & 255u;
                if (to < d.out_bytes) d.out[to] = static_cast<uint8_t>(b);
                ++to;
                if (b == 255u) {
                    if (to < d.out_bytes) d.out[to] = 0;
                    ++to;
                }
            }
    }
    if (4u * w + valid == d.nbytes && to + 2u <= d.out_bytes) {  // behind the last byte: EOI
        d.out[to] = 0xFF;
        d.out[to + 1] = 0xD9;
    }
}

struct HuffEncSet {
    rn_table<HuffEncDev> desc;         // [max_batch]
    rn_table<ImgOut> res;              // [max_batch]: zeros go up, the totals and statuses come down
};

struct HuffEncState {
    HuffEncSet set[2];
    rn_rotation turn;
    Tables* d_tables = nullptr;
    int16_t* d_coef = nullptr;         // rn_jpeg_huffenc_batch's uploads
    uint32_t* d_bits = nullptr;
    uint32_t* d_sums = nullptr;
    uint32_t* d_raw = nullptr;
    uint8_t* d_out = nullptr;
    size_t coef_cap = 0, bits_cap = 0, sums_cap = 0, raw_cap = 0, out_cap = 0;
    hipEvent_t stuffed = nullptr;
    rn_timer timer[3];                 // the launches in front of the first read, between the reads, behind the second
    bool ready = false;
};

int huffenc_state(rn_handle* h, HuffEncState** out) {
    if (!h->jpeg_huffenc) {
        HuffEncState* s = new HuffEncState();
        h->jpeg_huffenc = s;           // (rn_jpeg_huffenc_release frees whatever of it exists)
        const size_t nb = static_cast<size_t>(h->max_batch);
        int rc;
        for (HuffEncSet& e : s->set)
            if ((rc = e.desc.alloc(nb)) != RN_OK || (rc = e.res.alloc(nb)) != RN_OK) return rc;
        if ((rc = s->turn.create()) != RN_OK) return rc;
        for (rn_timer& t : s->timer)
            if ((rc = t.create()) != RN_OK) return rc;
        RN_HIP(hipEventCreateWithFlags(&s->stuffed, hipEventDisableTiming));
        Tables tables;
        build_tables(&tables);
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&s->d_tables), sizeof(Tables)));
        RN_HIP(hipMemcpy(s->d_tables, &tables, sizeof(Tables), hipMemcpyHostToDevice));
        s->ready = true;
    }
    *out = static_cast<HuffEncState*>(h->jpeg_huffenc);
    if (!(*out)->ready) {
        rn_set_error("rn_jpeg_huffenc: the stage's state could not be allocated earlier");
        return RN_E_STATE;
    }
    if (!h->copy_stream) RN_HIP(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    return RN_OK;
}

// results of the batch's launches so far -> the set's host array; waits
int read_results(rn_handle* h, HuffEncSet& sl, int n) {
    RN_HIP(hipMemcpyAsync(sl.res.host, sl.res.dev, static_cast<size_t>(n) * sizeof(ImgOut), hipMemcpyDeviceToHost, h->stream));
    RN_HIP(hipStreamSynchronize(h->stream));
    return RN_OK;
}

// The four phases on coefficients in device memory (d_coef[i]: image i's, rn_jpeg_coeff_count elements; ordered on the handle's
// stream) into files[i].  status[i] holds RN_JPEG_ENC_ST_TOO_LARGE where the caller decided it; those images are skipped.
int huffenc_run(rn_handle* h, HuffEncState* st, const rn_jpeg_info* const* infos, int16_t* const* d_coef, int n, uint8_t* const* files,
                const size_t* caps, size_t* lens, int32_t* status) {
    int rc, set;
    if ((rc = st->turn.acquire(&set)) != RN_OK) return rc;
    HuffEncSet& sl = st->set[set];
    for (rn_timer& t : st->timer) t.timed = false;
    // ---- lengths and offsets
    size_t blocks_total = 0, sums_total = 0;
    uint32_t max_blocks = 0, max_sums = 0;
    for (int i = 0; i < n; ++i) {
        HuffEncDev& d = sl.desc.host[i];
        std::memset(&d, 0, sizeof(d));
        std::memset(&sl.res.host[i], 0, sizeof(ImgOut));
        lens[i] = 0;
        if (status[i] != RN_JPEG_ENC_ST_OK) continue;
        const rn_jpeg_info& f = *infos[i];
        d.nblocks = static_cast<uint32_t>(rn_jpeg::coeff_count(f) / 64);      // <= RN_JPEG_HUFFENC_MAX_BLOCKS
        d.mcus_x = static_cast<uint32_t>(f.blocks_w[1]);
        d.nsums = (d.nblocks + kScanTile - 1) / kScanTile;
        d.rounds = (d.nsums + kWg - 1) / kWg;
        blocks_total += d.nblocks;
        sums_total += d.nsums;
        max_blocks = std::max(max_blocks, d.nblocks);
        max_sums = std::max(max_sums, d.nsums);
    }
    if (max_blocks == 0) return RN_OK;                           // (every image was too large: nothing is enqueued)
    if ((rc = rn_grow_scratch(h, &st->d_bits, &st->bits_cap, blocks_total, "JPEG Huffman-encode bit counts")) != RN_OK) return rc;
    if ((rc = rn_grow_scratch(h, &st->d_sums, &st->sums_cap, sums_total, "JPEG Huffman-encode tile sums")) != RN_OK) return rc;
    size_t block_off = 0, sum_off = 0;
    for (int i = 0; i < n; ++i) {
        HuffEncDev& d = sl.desc.host[i];
        if (!d.nblocks) continue;
        const rn_jpeg_info& f = *infos[i];
        size_t off = 0;
        for (int c = 0; c < 3; ++c) {
            d.coef[c] = d_coef[i] + off;
            off += static_cast<size_t>(f.blocks_w[c]) * f.blocks_h[c] * 64;
        }
        d.bits = st->d_bits + block_off;
        d.sums = st->d_sums + sum_off;
        d.res = sl.res.dev + i;
        block_off += d.nblocks;
        sum_off += d.nsums;
    }
    const size_t un = static_cast<size_t>(n);
    if ((rc = sl.desc.upload(un, h->stream)) != RN_OK || (rc = sl.res.upload(un, h->stream)) != RN_OK) return rc;
    if ((rc = st->timer[0].start(h->stream)) != RN_OK) return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(huffenc_lengths_kernel, dim3((max_blocks + kWaves - 1) / kWaves, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev, st->d_tables);
    RN_CHECK_LAUNCH();
    hipLaunchKernelGGL(huffenc_sum_tiles_kernel, dim3(max_sums, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev);
    RN_CHECK_LAUNCH();
    hipLaunchKernelGGL(huffenc_scan_sums_kernel, dim3(n), dim3(kWg), 0, h->stream, sl.desc.dev, 2);
    RN_CHECK_LAUNCH();
    hipLaunchKernelGGL(huffenc_scan_tiles_kernel, dim3(max_sums, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev);
    RN_CHECK_LAUNCH();
    if ((rc = st->timer[0].stop(h->stream)) != RN_OK) return rc;
    if ((rc = read_results(h, sl, n)) != RN_OK) return rc;
    // ---- the unstuffed stream at its real size: scatter, count
    size_t raw_total = 0;
    max_blocks = max_sums = 0;
    sums_total = 0;
    for (int i = 0; i < n; ++i) {
        HuffEncDev& d = sl.desc.host[i];
        if (!d.nblocks) continue;
        if (sl.res.host[i].status != RN_JPEG_ENC_ST_OK) {
            status[i] = sl.res.host[i].status;
            d.nblocks = 0;
            continue;
        }
        d.total_bits = sl.res.host[i].total_bits;
        d.nbytes = (d.total_bits + 7) / 8;                       // < 2^29
        d.raw_words = d.nbytes / 4 + 1;
        d.nsums = (d.nbytes + kStuffChunk - 1) / kStuffChunk;
        d.rounds = (d.nsums + kWg - 1) / kWg;
        raw_total += d.raw_words;
        sums_total += d.nsums;
        max_blocks = std::max(max_blocks, d.nblocks);
        max_sums = std::max(max_sums, d.nsums);
    }
    if (max_blocks) {
        if ((rc = rn_grow_scratch(h, &st->d_raw, &st->raw_cap, raw_total, "JPEG Huffman-encode unstuffed stream")) != RN_OK) return rc;
        if ((rc = rn_grow_scratch(h, &st->d_sums, &st->sums_cap, sums_total, "JPEG Huffman-encode chunk counts")) != RN_OK) return rc;
        size_t raw_off = 0;
        sum_off = 0;
        for (int i = 0; i < n; ++i) {
            HuffEncDev& d = sl.desc.host[i];
            if (!d.nblocks) continue;
            d.raw = st->d_raw + raw_off;
            d.sums = st->d_sums + sum_off;
            raw_off += d.raw_words;
            sum_off += d.nsums;
        }
        if ((rc = sl.desc.upload(un, h->stream)) != RN_OK) return rc;
        RN_HIP(hipMemsetAsync(st->d_raw, 0, raw_total * sizeof(uint32_t), h->stream));
        if ((rc = st->timer[1].start(h->stream)) != RN_OK) return rc;
        hipLaunchKernelGGL(huffenc_scatter_kernel, dim3((max_blocks + kWaves - 1) / kWaves, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev, st->d_tables);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(huffenc_count_ff_kernel, dim3(max_sums, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev);
        RN_CHECK_LAUNCH();
        hipLaunchKernelGGL(huffenc_scan_sums_kernel, dim3(n), dim3(kWg), 0, h->stream, sl.desc.dev, 4);
        RN_CHECK_LAUNCH();
        if ((rc = st->timer[1].stop(h->stream)) != RN_OK) return rc;
        if ((rc = read_results(h, sl, n)) != RN_OK) return rc;
    }
    // ---- the stuffed stream at its real size, for the images whose file fits its buffer
    size_t out_total = 0;
    max_sums = 0;
    for (int i = 0; i < n; ++i) {
        HuffEncDev& d = sl.desc.host[i];
        if (!d.nblocks) continue;
        const size_t scan = static_cast<size_t>(d.nbytes) + sl.res.host[i].total_ff + 2;      // < 2^30 + 2
        lens[i] = rn_jpeg::kEncHeaderBytes + scan;
        if (lens[i] > caps[i]) {
            status[i] = RN_JPEG_ENC_ST_CAP;
            d.nblocks = 0;
            continue;
        }
        d.out_bytes = static_cast<uint32_t>(scan);
        out_total += (scan + 3) & ~static_cast<size_t>(3);
        max_sums = std::max(max_sums, d.nsums);
    }
    if (max_sums) {
        if ((rc = rn_grow_scratch(h, &st->d_out, &st->out_cap, out_total, "JPEG Huffman-encode stuffed stream")) != RN_OK) return rc;
        size_t out_off = 0;
        for (int i = 0; i < n; ++i) {
            HuffEncDev& d = sl.desc.host[i];
            if (!d.nblocks) continue;
            d.out = st->d_out + out_off;
            out_off += (static_cast<size_t>(d.out_bytes) + 3) & ~static_cast<size_t>(3);
        }
        if ((rc = sl.desc.upload(un, h->stream)) != RN_OK) return rc;
        if ((rc = st->timer[2].start(h->stream)) != RN_OK) return rc;
        hipLaunchKernelGGL(huffenc_stuff_kernel, dim3(max_sums, 1, n), dim3(kWg), 0, h->stream, sl.desc.dev);
        RN_CHECK_LAUNCH();
        if ((rc = st->timer[2].stop(h->stream)) != RN_OK) return rc;
        // the headers are written while the launch runs; the scans come down behind them on the copy stream
        RN_HIP(hipEventRecord(st->stuffed, h->stream));
        RN_HIP(hipStreamWaitEvent(h->copy_stream, st->stuffed, 0));
        for (int i = 0; i < n; ++i) {
            const HuffEncDev& d = sl.desc.host[i];
            if (!d.nblocks) continue;
            rn_jpeg::ByteWriter w{files[i], caps[i]};
            rn_jpeg::write_headers(*infos[i], w);
            RN_HIP(hipMemcpyAsync(files[i] + rn_jpeg::kEncHeaderBytes, d.out, d.out_bytes, hipMemcpyDeviceToHost, h->copy_stream));
        }
        RN_HIP(hipStreamSynchronize(h->copy_stream));
    }
    return st->turn.retire(h->stream);
}

int check_outputs(const char* who, uint8_t* const* files, const size_t* caps, size_t* lens, int32_t* status, int n) {
    if (!files || !caps || !lens || !status) {
        rn_set_error("%s: null argument", who);
        return RN_E_INVALID;
    }
    for (int i = 0; i < n; ++i)
        if (!files[i] && caps[i]) {
            rn_set_error("%s: image %d has no output buffer", who, i);
            return RN_E_INVALID;
        }
    return RN_OK;
}

}  // namespace

void rn_jpeg_huffenc_release(rn_handle* h) {
    HuffEncState* s = static_cast<HuffEncState*>(h->jpeg_huffenc);
    if (!s) return;
    for (void* p : {static_cast<void*>(s->d_tables), static_cast<void*>(s->d_coef), static_cast<void*>(s->d_bits), static_cast<void*>(s->d_sums),
                    static_cast<void*>(s->d_raw), static_cast<void*>(s->d_out)})
        if (p) (void)hipFree(p);
    if (s->stuffed) (void)hipEventDestroy(s->stuffed);
    delete s;                          // (the tables, their rotation and the timers free themselves)
    h->jpeg_huffenc = nullptr;
}

extern "C" int rn_jpeg_encode_headers(const rn_jpeg_info* info, uint8_t* out, size_t cap, size_t* len) {
    const char* why = "";
    const int rc = rn_jpeg_huffenc::encode_headers(info, out, cap, len, &why);
    if (rc != RN_OK) rn_set_error("rn_jpeg_encode_headers: %s", why);
    return rc;
}

extern "C" int rn_jpeg_huffenc_model(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len, int32_t* status) {
    const char* why = "";
    const int rc = rn_jpeg_huffenc::model(info, coeffs, out, cap, len, status, &why);
    if (rc != RN_OK) rn_set_error("rn_jpeg_huffenc_model: %s", why);
    return rc;
}

extern "C" int rn_jpeg_huffenc_batch(rn_handle* h, const rn_jpeg_info* infos, const int16_t* const* coeffs_host, int n, uint8_t* const* files,
                                     const size_t* caps, size_t* lens, int32_t* status) {
    const char* who = "rn_jpeg_huffenc_batch";
    int rc = rn_check_batch(who, h, infos, n);
    if (rc != RN_OK) return rc;
    if (!coeffs_host) {
        rn_set_error("%s: null argument", who);
        return RN_E_INVALID;
    }
    if ((rc = check_outputs(who, files, caps, lens, status, n)) != RN_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (!rn_jpeg::encode_info_ok(infos[i]) || !coeffs_host[i]) {
            rn_set_error("%s: image %d: %s", who, i, coeffs_host[i] ? "the info is not one rn_jpeg_encode_info fills" : "no coefficients");
            return RN_E_INVALID;
        }
    DeviceGuard guard(h->device);
    HuffEncState* st = nullptr;
    if ((rc = huffenc_state(h, &st)) != RN_OK) return rc;
    std::vector<const rn_jpeg_info*> info_of(n);
    std::vector<int16_t*> d_coef(n, nullptr);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        info_of[i] = &infos[i];
        status[i] = too_large(infos[i]) ? RN_JPEG_ENC_ST_TOO_LARGE : RN_JPEG_ENC_ST_OK;      // (from the info alone)
        if (status[i] == RN_JPEG_ENC_ST_OK) total += rn_jpeg::coeff_count(infos[i]);
    }
    if ((rc = rn_grow_scratch(h, &st->d_coef, &st->coef_cap, total, "JPEG Huffman-encode coefficients")) != RN_OK) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        if (status[i] != RN_JPEG_ENC_ST_OK) continue;
        const size_t count = rn_jpeg::coeff_count(infos[i]);
        d_coef[i] = st->d_coef + off;
        RN_HIP(hipMemcpyAsync(d_coef[i], coeffs_host[i], count * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
        off += count;
    }
    return huffenc_run(h, st, info_of.data(), d_coef.data(), n, files, caps, lens, status);
}

extern "C" int rn_jpeg_encode_files_device(rn_handle* h, const rn_jpeg_source* srcs, int n, uint8_t* const* files, const size_t* caps,
                                           size_t* lens, int32_t* status) {
    const char* who = "rn_jpeg_encode_files_device";
    int rc = rn_jpeg_enc_check(who, h, srcs, n);
    if (rc != RN_OK) return rc;
    if ((rc = check_outputs(who, files, caps, lens, status, n)) != RN_OK) return rc;
    DeviceGuard guard(h->device);
    HuffEncState* st = nullptr;
    if ((rc = huffenc_state(h, &st)) != RN_OK) return rc;
    // the images that take part, in order: an image that is too large gets no launch at all
    std::vector<rn_jpeg_source> part;
    std::vector<int> index;
    std::vector<const rn_jpeg_info*> info_of(n);
    for (int i = 0; i < n; ++i) {
        info_of[i] = &srcs[i].info;
        status[i] = too_large(srcs[i].info) ? RN_JPEG_ENC_ST_TOO_LARGE : RN_JPEG_ENC_ST_OK;
        lens[i] = 0;
        if (status[i] == RN_JPEG_ENC_ST_OK) {
            part.push_back(srcs[i]);
            index.push_back(i);
        }
    }
    if (part.empty()) return RN_OK;
    std::vector<int16_t*> part_coef(part.size(), nullptr), d_coef(n, nullptr);
    if ((rc = rn_jpeg_enc_pixels(h, part.data(), static_cast<int>(part.size()), part_coef.data())) != RN_OK) return rc;
    for (size_t k = 0; k < part.size(); ++k) d_coef[index[k]] = part_coef[k];
    return huffenc_run(h, st, info_of.data(), d_coef.data(), n, files, caps, lens, status);
}

extern "C" int rn_jpeg_last_huffenc_ms(rn_handle* h, float* ms) {
    const char* who = "rn_jpeg_last_huffenc_ms";
    const HuffEncState* st = h ? static_cast<const HuffEncState*>(h->jpeg_huffenc) : nullptr;
    float sum = 0.f;
    for (int k = 0; k < 3; ++k) {
        if (k > 0 && st && !st->timer[k].timed) continue;        // (a batch whose images all stopped at a read has no later launches)
        float part = 0.f;
        const int rc = rn_timer::read(who, h, st ? &st->timer[k] : nullptr, "no batch has been Huffman-encoded on this handle", h ? h->device : 0, &part);
        if (rc != RN_OK) return rc;
        sum += part;
    }
    *ms = sum;
    return RN_OK;
}
