// The Huffman ENCODE step of baseline JPEG, written once for host and device.  It is encode_one_block of
// rn_jpeg_host.h's entropy_encode restated without the streaming accumulator: what a block contributes to the scan is a pure
// function of its 64 coefficients and of the DC of the block in front of it in its component, and what ZIGZAG POSITION k of the
// block contributes (`piece`) is a pure function of the value there and of the 64-bit mask of the block's non-zero positions:
//   k = 0      the DC category code and the magnitude bits of the DC difference
//   k >= 1     nothing for a zero; else the ZRLs of the zero run in front (the distance to the set bit below k), the run/size
//              code and the magnitude bits: at most 3 x 11 + 16 + 10 = 59 bits, one 64-bit value
//   k = 63     EOB when the value there is zero (the block then ends in zeros)
// The pieces in order of k are the block's symbols, their lengths sum to the block's bit count, and a block's bits start where
// the exclusive scan of the counts in scan (MCU) order puts them.  On the GPU a lane is a zigzag position and a wave a block
// (rn_jpeg_huffenc.hip); the host model further down runs the same phases, work item after work item, through these functions.
// Every function above the model is __host__ __device__; compiled as plain C++ the file includes no HIP header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rn_jpeg_host.h"

#if defined(__HIPCC__)
#define RN_HD __host__ __device__
#else
#define RN_HD
#endif

namespace rn_jpeg_huffenc {

constexpr int kMaxPieceBits = 3 * 11 + 16 + 10;                    // 59: three ZRLs of the luma table, a 16-bit code, category 10
constexpr int kMaxBlockBits = 9 + 11 + 63 * 26;                    // 1658: the worst case beside rn_jpeg::kEncBlockBytes
static_assert(rn_jpeg::kEncBlockBytes == 2 * ((kMaxBlockBits + 7) / 8), "the same worst case");
static_assert(RN_JPEG_HUFFENC_MAX_BLOCKS == 0xFFFFFFFFu / kMaxBlockBits, "bit offsets of an image stay inside 32 bits");
constexpr uint32_t kScanTile = 256;                                // block counts one workgroup scans
constexpr uint32_t kStuffChunk = 1024;                             // unstuffed bytes one workgroup stuffs (a dword per lane)

// The Annex K code / size tables of the file's two table classes (0: luma, 1: chroma), and zigzag -> natural.
struct Tables {
    uint16_t dc_code[2][16];           // [category]; 12 .. 15 have no code (size 0)
    uint16_t ac_code[2][256];          // [(run << 4) | category]
    uint8_t dc_size[2][16];
    uint8_t ac_size[2][256];
    uint8_t natural[64];
};

inline void build_tables(Tables* t) {
    std::memset(t, 0, sizeof(*t));
    for (int c = 0; c < 2; ++c) {
        rn_jpeg::EncTable e;
        rn_jpeg::build_enc_table(rn_jpeg::kStdDcBits[c], rn_jpeg::kStdDcVals, e);
        for (int s = 0; s < 16; ++s) {
            t->dc_code[c][s] = e.code[s];
            t->dc_size[c][s] = e.size[s];
        }
        rn_jpeg::build_enc_table(rn_jpeg::kStdAcBits[c], rn_jpeg::kStdAcVals[c], e);
        std::memcpy(t->ac_code[c], e.code, sizeof(e.code));
        std::memcpy(t->ac_size[c], e.size, sizeof(e.size));
    }
    std::memcpy(t->natural, rn_jpeg::kNatural, sizeof(t->natural));
}

RN_HD inline int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// Where block s of the scan (MCU order, 4:2:0: four luma blocks, Cb, Cr per MCU) lies: its component, its block index inside
// the component ([block_y][block_x]) and the index of the block whose DC is its predictor (-1: the predictor is 0).
struct Where {
    int32_t comp;
    int64_t block, pred;
};
RN_HD inline Where locate(uint32_t mcus_x, uint32_t s) {
    const uint32_t mcu = s / 6u, k = s - mcu * 6u;
    if (k >= 4u) return Where{static_cast<int32_t>(k) - 3, static_cast<int64_t>(mcu), static_cast<int64_t>(mcu) - 1};
    const uint32_t my = mcu / mcus_x, mx = mcu - my * mcus_x;
    const int64_t bw = 2 * static_cast<int64_t>(mcus_x);
    const int64_t at = (2 * static_cast<int64_t>(my) + (k >> 1)) * bw + 2 * mx + (k & 1u);
    int64_t pred;
    if (k == 1u || k == 3u) {
        pred = at - 1;
    } else if (k == 2u) {
        pred = at - bw + 1;                                     // the right-hand block of the MCU's top row
    } else if (mcu == 0u) {
        pred = -1;
    } else {
        const uint32_t pm = mcu - 1u, py = pm / mcus_x, px = pm - py * mcus_x;
        pred = (2 * static_cast<int64_t>(py) + 1) * bw + 2 * px + 1;       // block 3 of the MCU in front
    }
    return Where{0, at, pred};
}

// What one zigzag position contributes: `len` bits, right-aligned in `v`, first bit first.
struct Piece {
    uint64_t v;
    uint32_t len;
    int32_t status;                    // RN_JPEG_ENC_ST_OK or RN_JPEG_ENC_ST_CATEGORY (then len = 0)
};

// tab: the table class.  val: the DC DIFFERENCE for k = 0, else the coefficient at zigzag k.  nonzero: bit j set where the
// coefficient at zigzag j is not 0, j = 1 .. 63 (bit 0 is ignored).
RN_HD inline Piece piece(const Tables& t, int tab, int k, int val, uint64_t nonzero) {
    const uint32_t a = static_cast<uint32_t>(val < 0 ? -val : val);
    const int n = bit_length(a);
    if (k == 0) {
        if (n > 11) return Piece{0, 0, RN_JPEG_ENC_ST_CATEGORY};
        const uint32_t mag = static_cast<uint32_t>(val < 0 ? val - 1 : val) & ((1u << n) - 1u);
        return Piece{(static_cast<uint64_t>(t.dc_code[tab][n]) << n) | mag, static_cast<uint32_t>(t.dc_size[tab][n]) + n, RN_JPEG_ENC_ST_OK};
    }
    if (val == 0) {
        if (k == 63) return Piece{t.ac_code[tab][0x00], t.ac_size[tab][0x00], RN_JPEG_ENC_ST_OK};       // EOB
        return Piece{0, 0, RN_JPEG_ENC_ST_OK};
    }
    if (n > 10) return Piece{0, 0, RN_JPEG_ENC_ST_CATEGORY};
    // the zero run in front: the distance to the set bit below k, position 0 (the DC) standing for "none"
    const uint64_t below = (nonzero | 1ull) & ((1ull << k) - 1ull);
    const int run = k - (63 - __builtin_clzll(below)) - 1;
    uint64_t v = 0;
    uint32_t len = 0;
    for (int z = 0; z < 3; ++z)
        if (z < (run >> 4)) {
            v = (v << t.ac_size[tab][0xF0]) | t.ac_code[tab][0xF0];     // ZRL
            len += t.ac_size[tab][0xF0];
        }
    const int sym = ((run & 15) << 4) | n;
    const uint32_t mag = static_cast<uint32_t>(val < 0 ? val - 1 : val) & ((1u << n) - 1u);
    v = (((v << t.ac_size[tab][sym]) | t.ac_code[tab][sym]) << n) | mag;
    len += static_cast<uint32_t>(t.ac_size[tab][sym]) + n;
    return Piece{v, len, RN_JPEG_ENC_ST_OK};
}

RN_HD inline uint64_t nonzero_mask(const Tables& t, const int16_t* blk) {
    uint64_t m = 0;
    for (int k = 1; k < 64; ++k)
        if (blk[t.natural[k]] != 0) m |= 1ull << k;
    return m;
}

// A block's pieces in order (out[64], may be null) and its bit count.  blk: natural order; pred: the DC in front of it.
RN_HD inline uint32_t block_pieces(const Tables& t, int tab, const int16_t* blk, int pred, Piece* out, int32_t* status) {
    const uint64_t mask = nonzero_mask(t, blk);
    uint32_t bits = 0;
    for (int k = 0; k < 64; ++k) {
        const Piece p = piece(t, tab, k, k == 0 ? blk[0] - pred : blk[t.natural[k]], mask);
        if (p.status > *status) *status = p.status;
        if (out) out[k] = p;
        bits += p.len;
    }
    return bits;
}

// The `len` low bits of v into a stream of 32-bit words whose bit p is bit 31 - (p & 31) of word p >> 5 (a word is stored with
// its bytes swapped: the stream is big-endian).  At most three words; `merge(word index, bits)` ORs.
template <typename Merge>
RN_HD inline void put_bits(uint32_t pos, uint64_t v, uint32_t len, Merge&& merge) {
    for (int i = 0; i < 3; ++i)
        if (len > 0) {
            const uint32_t room = 32u - (pos & 31u), take = len < room ? len : room;
            const uint32_t chunk = static_cast<uint32_t>((v >> (len - take)) & ((1ull << take) - 1ull));
            merge(pos >> 5, chunk << (room - take));
            pos += take;
            len -= take;
        }
}

RN_HD inline uint32_t byte_swap(uint32_t w) { return __builtin_bswap32(w); }

// FF bytes among the first `valid` (1 .. 4) bytes of a dword of the unstuffed stream as memory holds it
RN_HD inline uint32_t count_ff(uint32_t word, uint32_t valid) {
    uint32_t n = 0;
    for (uint32_t j = 0; j < 4; ++j)
        if (j < valid && ((word >> (8 * j)) & 255u) == 255u) ++n;
    return n;
}

inline bool too_large(const rn_jpeg_info& f) { return rn_jpeg::coeff_count(f) / 64 > RN_JPEG_HUFFENC_MAX_BLOCKS; }

// rn_jpeg_encode_headers: SOI .. SOS for an info rn_jpeg_encode_info fills, bounded by cap.  The bytes come from
// rn_jpeg::write_headers, the one place the header is written (entropy_encode and the GPU call's host half call it too).
inline int encode_headers(const rn_jpeg_info* info, uint8_t* out, size_t cap, size_t* len, const char** why) {
    *why = "";
    if (!info || !len || (!out && cap)) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    *len = 0;
    if (!rn_jpeg::encode_info_ok(*info)) {
        *why = "the info is not one rn_jpeg_encode_info fills (3 components, 4:2:0, whole-MCU grids, 8-bit tables)";
        return RN_E_INVALID;
    }
    rn_jpeg::ByteWriter w{out, cap};
    rn_jpeg::write_headers(*info, w);
    *len = w.pos;
    if (w.pos > cap) {
        *why = "output buffer too small";
        return RN_E_RANGE;
    }
    return RN_OK;
}

// ---- the host model: the four phases of rn_jpeg_huffenc.hip, one work item after another -------------------------------------
// Arguments as rn_jpeg_entropy_encode takes them and refused the same way, except that what it refuses in the COEFFICIENTS and a
// short buffer are statuses: RN_OK with *status set.  Nothing is stored past cap.
inline int model(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len, int32_t* status, const char** why) {
    *why = "";
    if (!info || !coeffs || !len || !status || (!out && cap)) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    *len = 0;
    *status = RN_JPEG_ENC_ST_OK;
    if (!rn_jpeg::encode_info_ok(*info)) {
        *why = "the info is not one rn_jpeg_encode_info fills (3 components, 4:2:0, whole-MCU grids, 8-bit tables)";
        return RN_E_INVALID;
    }
    const rn_jpeg_info& f = *info;
    if (too_large(f)) {                                          // (from the info alone: the coefficients are not read)
        *status = RN_JPEG_ENC_ST_TOO_LARGE;
        return RN_OK;
    }
    static thread_local Tables tables;
    static thread_local bool built = false;
    if (!built) {
        build_tables(&tables);
        built = true;
    }
    const uint32_t mcus_x = static_cast<uint32_t>(f.blocks_w[1]);
    const uint32_t nblocks = static_cast<uint32_t>(rn_jpeg::coeff_count(f) / 64);
    const int16_t* base[3];
    size_t off = 0;
    for (int c = 0; c < 3; ++c) {
        base[c] = coeffs + off;
        off += static_cast<size_t>(f.blocks_w[c]) * f.blocks_h[c] * 64;
    }
    auto block_of = [&](uint32_t s, const int16_t** blk, int* pred, int* tab) {
        const Where at = locate(mcus_x, s);
        *blk = base[at.comp] + at.block * 64;
        *pred = at.pred < 0 ? 0 : base[at.comp][at.pred * 64];
        *tab = at.comp ? 1 : 0;
    };
    // 1: lengths
    std::vector<uint32_t> bits(nblocks);
    for (uint32_t s = 0; s < nblocks; ++s) {
        const int16_t* blk;
        int pred, tab;
        block_of(s, &blk, &pred, &tab);
        bits[s] = block_pieces(tables, tab, blk, pred, nullptr, status);
    }
    if (*status != RN_JPEG_ENC_ST_OK) return RN_OK;
    // 2: offsets, tile by tile as the launches do: the tiles' sums, their scan, the scan inside each tile
    const uint32_t ntiles = (nblocks + kScanTile - 1) / kScanTile;
    std::vector<uint32_t> tile(ntiles, 0);
    for (uint32_t s = 0; s < nblocks; ++s) tile[s / kScanTile] += bits[s];
    uint32_t total_bits = 0;
    for (uint32_t i = 0; i < ntiles; ++i) {
        const uint32_t sum = tile[i];
        tile[i] = total_bits;
        total_bits += sum;
    }
    for (uint32_t i = 0; i < ntiles; ++i) {
        uint32_t run = tile[i];
        for (uint32_t s = i * kScanTile; s < nblocks && s < (i + 1) * kScanTile; ++s) {
            const uint32_t b = bits[s];
            bits[s] = run;
            run += b;
        }
    }
    // 3: scatter into the zeroed unstuffed stream; the last byte is padded with 1-bits
    const uint32_t nbytes = (total_bits + 7) / 8;
    std::vector<uint32_t> raw(nbytes / 4 + 1, 0);               // as memory holds it: bytes swapped
    auto merge = [&](uint32_t w, uint32_t v) { raw[w] |= byte_swap(v); };
    Piece pieces[64];
    for (uint32_t s = 0; s < nblocks; ++s) {
        const int16_t* blk;
        int pred, tab;
        block_of(s, &blk, &pred, &tab);
        block_pieces(tables, tab, blk, pred, pieces, status);
        uint32_t pos = bits[s];
        for (int k = 0; k < 64; ++k) {
            put_bits(pos, pieces[k].v, pieces[k].len, merge);
            pos += pieces[k].len;
        }
    }
    const uint32_t pad = (8u - (total_bits & 7u)) & 7u;
    put_bits(total_bits, (1u << pad) - 1u, pad, merge);
    // 4: FF counts per chunk, their scan, byte i to i + (#FF in front of it) with 00 behind every FF, then EOI
    const uint32_t nchunks = (nbytes + kStuffChunk - 1) / kStuffChunk;
    std::vector<uint32_t> ff(nchunks, 0);
    auto valid_of = [&](uint32_t w) { return nbytes - 4 * w < 4u ? nbytes - 4 * w : 4u; };
    for (uint32_t w = 0; 4 * static_cast<size_t>(w) < nbytes; ++w) ff[4 * w / kStuffChunk] += count_ff(raw[w], valid_of(w));
    uint32_t total_ff = 0;
    for (uint32_t i = 0; i < nchunks; ++i) {
        const uint32_t sum = ff[i];
        ff[i] = total_ff;
        total_ff += sum;
    }
    size_t header = 0;
    int rc = encode_headers(info, out, cap, &header, why);
    if (rc != RN_OK && rc != RN_E_RANGE) return rc;
    *why = "";
    *len = header + nbytes + total_ff + 2;
    if (*len > cap) {
        *status = RN_JPEG_ENC_ST_CAP;
        return RN_OK;
    }
    uint8_t* scan = out + header;
    for (uint32_t i = 0; i < nchunks; ++i) {
        uint32_t before = ff[i];
        for (uint32_t w = i * (kStuffChunk / 4); 4 * static_cast<size_t>(w) < nbytes && w < (i + 1) * (kStuffChunk / 4); ++w) {
            const uint32_t valid = valid_of(w);
            for (uint32_t j = 0; j < valid; ++j) {
                const uint8_t b = static_cast<uint8_t>(raw[w] >> (8 * j));
                scan[4 * static_cast<size_t>(w) + j + before] = b;
                if (b == 0xFF) scan[4 * static_cast<size_t>(w) + j + ++before] = 0;
            }
        }
    }
    scan[nbytes + total_ff] = 0xFF;
    scan[nbytes + total_ff + 1] = 0xD9;
    return RN_OK;
}

}  // namespace rn_jpeg_huffenc
