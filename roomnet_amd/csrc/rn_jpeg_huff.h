// The Huffman decode step of baseline JPEG, written once for host and device.  The arithmetic is
// rn_jpeg_host.h's decode_symbol / receive_extend -- the 9-bit first-level lookup, the canonical maxcode walk, FF 00 destuffing,
// EOB / ZRL, the RN_JPEG_COEF_LIMIT checks -- restated over a BIT POSITION in the scan instead of a streaming accumulator, so that
// a decoder can start anywhere: the parallel decode (rn_jpeg_huff.hip on the GPU, rn_jpeg_huff_model.h on the host) cuts the
// scan into subsequences of RN_JPEG_SUBSEQ_BYTES raw bytes, decodes each from a guessed state, and repeats from the neighbour's
// exit state until the chain of states is consistent; a chain that is consistent from subsequence 0 is the sequential decode.
// Every function is __host__ __device__; compiled as plain C++ the file includes no HIP header.  Every read of the scan is bounded
// by its length and nothing is indexed with a decoded value that was not checked first.
#pragma once
#include <cstddef>
#include <cstdint>

#include "roomnet_hip.h"

#if defined(__HIPCC__)
#define RN_HD __host__ __device__
#else
#define RN_HD
#endif

#define RN_JPEG_SUBSEQ_BYTES 128

namespace rn_jpeg_huff {

constexpr int kLookBits = 9;                    // rn_jpeg::kLookBits
constexpr int kGroup = 256;                     // subsequences of one workgroup: phase 2 runs inside groups first, then across them
constexpr uint32_t kMaxScanBytes = 1u << 24;    // a longer scan is RN_JPEG_ST_TOO_LARGE (bit positions stay far inside 32 bits)
constexpr int kMaxFill = 16;                    // FF fill bytes followed in front of a restart marker
constexpr uint32_t kInvalid = 0xFFFFFFFFu;

// What the kernels keep in LDS per image: the components' tables (rn_jpeg_scan), their quantisation tables, zigzag -> natural.
struct Tables {
    rn_jpeg_hufftab dc[3], ac[3];
    uint16_t qt[3][64];
    uint8_t natural[64];
};
static_assert(sizeof(Tables) % 4 == 0, "copied into LDS as dwords");

struct Geom {
    int32_t ncomp, hs, vs;
    int32_t mcus_x;            // MCUs per row
    int32_t bw[3];             // blocks per row of each component
    int32_t nslots;            // blocks per MCU: hs * vs + ncomp - 1
    int32_t total;             // blocks of the image, all components
    int32_t ri;                // restart interval in MCUs, 0: none
};

// Decoder state.  p: bit position in the scan, never inside the 00 of an FF 00 pair.  sk: (slot << 8) | k -- the slot inside the
// MCU, which selects component and tables, and the zigzag index, 0: a DC code is next -- or kInvalid: the decoder needed bits from
// beyond the end of the scan.  n: blocks completed since the decoder's entry.
struct State {
    uint32_t p, sk, n, pad;
};
RN_HD inline bool same(const State& a, const State& b) { return a.p == b.p && a.sk == b.sk && a.n == b.n; }
// the entry state of a subsequence: what the decoder of the one in front left, its block count started again
RN_HD inline State entry_of(const State& previous_exit) { return State{previous_exit.p, previous_exit.sk, 0, 0}; }

struct Ctx {
    const uint8_t* scan;
    uint32_t len;
    const Tables* t;
    Geom g;
};

RN_HD inline Geom geometry(const rn_jpeg_info& f) {
    Geom g;
    g.ncomp = f.ncomp;
    g.hs = f.hsamp;
    g.vs = f.vsamp;
    g.mcus_x = f.blocks_w[0] / (f.hsamp > 0 ? f.hsamp : 1);
    g.total = 0;
    for (int c = 0; c < 3; ++c) {
        g.bw[c] = c < f.ncomp ? f.blocks_w[c] : 0;
        if (c < f.ncomp) g.total += f.blocks_w[c] * f.blocks_h[c];
    }
    g.nslots = f.hsamp * f.vsamp + f.ncomp - 1;
    g.ri = f.restart_interval;
    return g;
}

// what the host decides before anything is launched
RN_HD inline int32_t precheck(uint64_t scan_len) {
    if (scan_len == 0) return RN_JPEG_ST_TRUNCATED;
    if (scan_len > kMaxScanBytes) return RN_JPEG_ST_TOO_LARGE;
    return RN_JPEG_ST_OK;
}

RN_HD inline int slot_component(const Geom& g, uint32_t slot) {
    const uint32_t luma = static_cast<uint32_t>(g.hs * g.vs);
    return slot < luma ? 0 : static_cast<int>(slot - luma) + 1;
}

// Block number b of the scan (b < g.total) -> its component and its place in the component's [block_y][block_x] grid.
RN_HD inline void block_place(const Geom& g, uint32_t b, int* comp, uint32_t* addr) {
    const uint32_t mcu = b / static_cast<uint32_t>(g.nslots), slot = b - mcu * static_cast<uint32_t>(g.nslots);
    const uint32_t my = mcu / static_cast<uint32_t>(g.mcus_x), mx = mcu - my * static_cast<uint32_t>(g.mcus_x);
    const uint32_t luma = static_cast<uint32_t>(g.hs * g.vs);
    if (slot < luma) {
        const uint32_t v = slot / static_cast<uint32_t>(g.hs), hh = slot - v * static_cast<uint32_t>(g.hs);
        *comp = 0;
        *addr = (my * static_cast<uint32_t>(g.vs) + v) * static_cast<uint32_t>(g.bw[0]) + mx * static_cast<uint32_t>(g.hs) + hh;
    } else {
        *comp = static_cast<int>(slot - luma) + 1;
        *addr = mcu;
    }
}

// Block j of component c in scan order -> its place in the component's grid, and the MCU it belongs to.
RN_HD inline uint32_t component_block(const Geom& g, int c, uint32_t j, uint32_t* mcu, bool* first_of_mcu) {
    if (c > 0) {
        *mcu = j;
        *first_of_mcu = true;
        return j;
    }
    const uint32_t luma = static_cast<uint32_t>(g.hs * g.vs);
    const uint32_t m = j / luma, s = j - m * luma;
    const uint32_t my = m / static_cast<uint32_t>(g.mcus_x), mx = m - my * static_cast<uint32_t>(g.mcus_x);
    const uint32_t v = s / static_cast<uint32_t>(g.hs), hh = s - v * static_cast<uint32_t>(g.hs);
    *mcu = m;
    *first_of_mcu = s == 0;
    return (my * static_cast<uint32_t>(g.vs) + v) * static_cast<uint32_t>(g.bw[0]) + mx * static_cast<uint32_t>(g.hs) + hh;
}

// One data byte at raw position b: its value and the position behind it, or false at a marker, a lone FF or the end of the data.
RN_HD inline bool data_byte(const uint8_t* s, uint32_t len, uint32_t b, uint32_t* value, uint32_t* next) {
    if (b >= len) return false;
    const uint32_t c = s[b];
    if (c != 0xFF) {
        *value = c;
        *next = b + 1;
        return true;
    }
    if (b + 1 < len && s[b + 1] == 0x00) {
        *value = 0xFF;
        *next = b + 2;
        return true;
    }
    return false;
}

// The 32 bits at bit position p, destuffed.  *real: how many of them lie in front of the next marker or the end of the data, the
// others are zeros; *stop: where the bytes ended when real < 32.
RN_HD inline uint32_t peek32(const uint8_t* s, uint32_t len, uint32_t p, int* real, uint32_t* stop) {
    uint32_t b = p >> 3;
    const int off = static_cast<int>(p & 7);
    uint64_t acc = 0;
    int have = 0;
    for (int i = 0; i < 5; ++i) {
        uint32_t v, next;
        if (!data_byte(s, len, b, &v, &next)) break;
        acc = (acc << 8) | v;
        have += 8;
        b = next;
    }
    *stop = b;
    acc <<= (40 - have);
    const int r = have - off;
    *real = r < 0 ? 0 : (r > 32 ? 32 : r);
    return static_cast<uint32_t>(acc >> (8 - off));
}

// p moved on by n bits that peek32 reported as real
RN_HD inline uint32_t advance(const uint8_t* s, uint32_t len, uint32_t p, int n) {
    uint32_t b = p >> 3;
    int total = static_cast<int>(p & 7) + n;
    while (total >= 8) {
        b += (b + 1 < len && s[b] == 0xFF && s[b + 1] == 0x00) ? 2 : 1;
        total -= 8;
    }
    return b * 8 + static_cast<uint32_t>(total);
}

// FF (FF)* Dn at raw position b: the position behind the marker and n
RN_HD inline bool restart_marker(const uint8_t* s, uint32_t len, uint32_t b, uint32_t* after, int* number, bool* too_long) {
    *too_long = false;
    uint32_t q = b;
    int fill = 0;
    while (q < len && s[q] == 0xFF && fill <= kMaxFill) {
        ++q;
        ++fill;
    }
    if (fill > kMaxFill) {
        *too_long = true;
        return false;
    }
    if (q == b || q >= len || s[q] < 0xD0 || s[q] > 0xD7) return false;
    *after = q + 1;
    *number = s[q] & 7;
    return true;
}

// one Huffman code in the window's leading bits: the symbol and the code's length, or -1
RN_HD inline int lookup(const rn_jpeg_hufftab& t, uint32_t w, int* length) {
    const uint32_t e = t.look[w >> (32 - kLookBits)];
    if (e) {
        *length = static_cast<int>(e >> 8);
        return static_cast<int>(e & 0xFF);
    }
    int l = kLookBits + 1;
    int32_t code = static_cast<int32_t>(w >> (32 - l));
    while (l <= 16 && code > t.maxcode[l]) {
        ++l;
        if (l <= 16) code = static_cast<int32_t>(w >> (32 - l));
    }
    if (l > 16) return -1;
    const int idx = code + t.valoff[l];
    if (idx < 0 || idx > 255) return -1;
    *length = l;
    return t.vals[idx];
}

// the s-bit field behind a code of l bits as a signed value (JPEG's EXTEND); 1 <= s <= 15, l + s <= 31
RN_HD inline int extend(uint32_t w, int l, int s) {
    const int v = static_cast<int>((w << l) >> (32 - s));
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The sink of the synchronisation passes: nothing.
struct NoSink {
    RN_HD bool finished(uint32_t) const { return false; }
    RN_HD void status(int32_t) {}
    RN_HD void dc(uint32_t, int) {}
    RN_HD void ac(uint32_t, int, int) {}
    RN_HD void restart(uint32_t, int, const uint8_t*, uint32_t) {}
    RN_HD void mcu_start(uint32_t, const uint8_t*, uint32_t, uint32_t) {}
};

// The coefficient writer of phase 3.  base: blocks of the scan in front of the lane's entry state.  AC values go to their natural
// position, the DC DIFFERENCE to index 0 (phase 4 sums them); a block number is checked against the image's total before it is
// turned into an address.
struct Writer {
    const Geom* g;
    const Tables* t;
    int16_t* coef[3];
    uint32_t base;
    int32_t st = RN_JPEG_ST_OK;

    RN_HD bool finished(uint32_t n) const { return base + n >= static_cast<uint32_t>(g->total); }
    RN_HD void status(int32_t code) {
        if (code > st) st = code;
    }
    RN_HD void dc(uint32_t n, int diff) {
        int comp;
        uint32_t addr;
        block_place(*g, base + n, &comp, &addr);
        coef[comp][static_cast<size_t>(addr) * 64] = static_cast<int16_t>(diff);
    }
    RN_HD void ac(uint32_t n, int k, int val) {
        int comp;
        uint32_t addr;
        block_place(*g, base + n, &comp, &addr);
        const int nat = t->natural[k];
        const int dq = val * static_cast<int>(t->qt[comp][nat]);
        if (dq > RN_JPEG_COEF_LIMIT || dq < -RN_JPEG_COEF_LIMIT) status(RN_JPEG_ST_COEF_LIMIT);
        coef[comp][static_cast<size_t>(addr) * 64 + nat] = static_cast<int16_t>(val);
    }
    RN_HD static bool behind_marker(const uint8_t* s, uint32_t p) {
        const uint32_t b = p >> 3;
        return (p & 7) == 0 && b >= 2 && s[b - 1] >= 0xD0 && s[b - 1] <= 0xD7 && s[b - 2] == 0xFF;
    }
    // a restart marker number `number` taken at an MCU boundary, the decoder at bit position p: after exactly ri MCUs, numbers
    // counting mod 8, and not a second marker directly behind one
    RN_HD void restart(uint32_t n, int number, const uint8_t* s, uint32_t p) {
        const uint32_t mcu = (base + n) / static_cast<uint32_t>(g->nslots);
        if (g->ri <= 0 || mcu == 0 || mcu % static_cast<uint32_t>(g->ri) != 0 ||
            number != static_cast<int>((mcu / static_cast<uint32_t>(g->ri) - 1) & 7) || behind_marker(s, p))
            status(RN_JPEG_ST_RESTART);
    }
    // An MCU begins at bit position p without a marker in front of the decoder: where one is due, it has just been passed.  If not,
    // the marker is missing -- unless one begins within the next 8 data bytes: the sequential pass reads up to 64 bits ahead and
    // drops what it holds at a restart, so it takes some damaged intervals that end a few bytes early; those go back to it.
    RN_HD void mcu_start(uint32_t n, const uint8_t* s, uint32_t len, uint32_t p) {
        const uint32_t mcu = (base + n) / static_cast<uint32_t>(g->nslots);
        if (g->ri <= 0 || mcu == 0 || mcu % static_cast<uint32_t>(g->ri) != 0) return;
        if (behind_marker(s, p)) return;
        uint32_t b = (p + 7) >> 3;
        for (int i = 0; i < 8; ++i) {
            uint32_t v, next;
            if (!data_byte(s, len, b, &v, &next)) break;
            b = next;
        }
        uint32_t after;
        int number;
        bool too_long;
        status(restart_marker(s, len, b, &after, &number, &too_long) ? RN_JPEG_ST_NOT_SYNCED : RN_JPEG_ST_RESTART);
    }
};

// Whole symbols (a code and its magnitude field) from `st` until the bit position is >= end_bit; the exit state.  Every iteration
// moves p forward by at least one bit or ends the loop, so the trip count is bounded by end_bit - p.
template <class Sink>
RN_HD inline State decode_subsequence(const Ctx& c, State st, uint32_t end_bit, Sink& sink) {
    const uint8_t* s = c.scan;
    const uint32_t len = c.len;
    while (st.sk != kInvalid && st.p < end_bit) {
        if (sink.finished(st.n)) break;
        uint32_t slot = st.sk >> 8, k = st.sk & 0xFF;
        int real;
        uint32_t stop;
        const uint32_t w = peek32(s, len, st.p, &real, &stop);
        // restart markers: FF Dn at the byte boundary ends the bits in front of it, the rest of the byte is padding
        bool rst = false, too_long = false;
        uint32_t after = 0;
        int number = 0;
        if (real < 32) rst = restart_marker(s, len, stop, &after, &number, &too_long);
        if (too_long) sink.status(RN_JPEG_ST_NOT_SYNCED);          // (more fill bytes than this decoder follows)
        if (st.sk == 0) {
            if (rst && real < 8) {                                   // (only the padding of the last byte is left)
                sink.restart(st.n, number, s, st.p);
                st.p = after * 8;
                continue;
            }
            sink.mcu_start(st.n, s, len, st.p);
        }
        const int comp = slot_component(c.g, slot);
        // A code no table has, or a run past 63, is an error of the file for the writer and a wrong guess for a speculating lane.
        // Neither stops the decoder -- a lane that stopped would pass `invalid` on to every lane behind it, and the chain would only
        // grow by one subsequence per round -- it steps over one bit, or ends the block, and goes on looking for the true state.
        // Nothing is indexed with the rejected value.
        int l = 0, total, sym;
        bool no_code = false;
        if (k == 0) {
            sym = lookup(c.t->dc[comp], w, &l);
            no_code = sym < 0 || sym > 15;
            total = l + sym;
        } else {
            sym = lookup(c.t->ac[comp], w, &l);
            no_code = sym < 0;
            total = l + (sym & 15);
        }
        if (no_code) {
            sink.status(RN_JPEG_ST_INVALID_CODE);
            total = 1;
        }
        if (total > real) {                                          // the symbol needs bits from beyond a marker or the end
            sink.status(RN_JPEG_ST_TRUNCATED);
            if (rst) {                                               // behind a restart marker every decoder is in the true state
                st.p = after * 8;
                st.sk = 0;
                continue;
            }
            st.sk = kInvalid;
            break;
        }
        bool block_done = false;
        if (no_code) {
            // (the state stays)
        } else if (k == 0) {
            sink.dc(st.n, sym ? extend(w, l, sym) : 0);
            k = 1;
        } else {
            const int r = sym >> 4, size = sym & 15;
            if (size == 0) {
                if (r != 15)
                    block_done = true;                               // EOB
                else
                    k += 16;                                         // ZRL
            } else {
                k += static_cast<uint32_t>(r);
                if (k > 63) {
                    sink.status(RN_JPEG_ST_RUN_PAST_BLOCK);
                } else {
                    sink.ac(st.n, static_cast<int>(k), extend(w, l, size));
                    ++k;
                }
            }
            if (k >= 64) block_done = true;
        }
        st.p = advance(s, len, st.p, total);
        if (block_done) {
            ++st.n;
            slot = slot + 1 == static_cast<uint32_t>(c.g.nslots) ? 0 : slot + 1;
            k = 0;
        }
        st.sk = (slot << 8) | k;
    }
    return st;
}

RN_HD inline uint32_t subseq_count(uint32_t scan_len, uint32_t subseq_bytes) { return (scan_len + subseq_bytes - 1) / subseq_bytes; }

RN_HD inline uint32_t subseq_end_bit(uint32_t scan_len, uint32_t subseq_bytes, uint32_t i) {
    const uint64_t e = static_cast<uint64_t>(i + 1) * subseq_bytes;
    return static_cast<uint32_t>(e < scan_len ? e : scan_len) * 8;
}

// Lane i's first guess: its own first byte, slot 0, k 0.  A start on the 00 of an FF 00 pair, or on the second byte of a restart
// marker, looks one byte back and steps over it.  Lane 0's is the true state.
RN_HD inline State guess(const uint8_t* s, uint32_t len, uint32_t subseq_bytes, uint32_t i) {
    uint32_t b = i * subseq_bytes;
    if (i > 0 && b < len && s[b - 1] == 0xFF && (s[b] == 0x00 || (s[b] >= 0xD0 && s[b] <= 0xD7))) ++b;
    return State{b * 8, 0, 0, 0};
}

// Phase 3's lane: subsequence i from its entry state -- the stored exit state of i - 1 -- with the writer; `stored` is what phase
// 2 left for i.  The lane's status: what the decode met, RN_JPEG_ST_NOT_SYNCED when its exit state is not the stored one, and for
// the last lane RN_JPEG_ST_TRUNCATED when the scan ends before the image's last block.
RN_HD inline int32_t write_lane(const Ctx& c, State entry, const State& stored, uint32_t end_bit, bool last, Writer& w) {
    if (w.base >= static_cast<uint32_t>(c.g.total)) return RN_JPEG_ST_OK;       // the image was complete in front of this lane
    entry.n = 0;
    const State out = decode_subsequence(c, entry, end_bit, w);
    if (w.finished(out.n)) return w.st;
    if (!same(out, stored)) w.status(RN_JPEG_ST_NOT_SYNCED);
    if (last && out.sk != kInvalid) w.status(RN_JPEG_ST_TRUNCATED);
    return w.st;
}

// Phase 4 for a run of one component's blocks in scan order: j in [j0, j1), `pred` the predictor in front of j0.  Returns the
// predictor behind the run; writes the DC values when `coef` is given and reports the two limit checks of the host pass.
RN_HD inline long long dc_run(const Geom& g, int comp, uint32_t j0, uint32_t j1, long long pred, int q0, int16_t* coef, int32_t* status,
                              bool* reset_seen) {
    for (uint32_t j = j0; j < j1; ++j) {
        uint32_t mcu;
        bool first;
        const uint32_t addr = component_block(g, comp, j, &mcu, &first);
        if (first && g.ri > 0 && mcu % static_cast<uint32_t>(g.ri) == 0) {
            pred = 0;
            if (reset_seen) *reset_seen = true;
        }
        int16_t* blk = coef + static_cast<size_t>(addr) * 64;
        if (status) {
            pred += blk[0];
            const long long dq = pred * q0;
            if (pred > RN_JPEG_COEF_LIMIT || pred < -RN_JPEG_COEF_LIMIT || dq > RN_JPEG_COEF_LIMIT || dq < -RN_JPEG_COEF_LIMIT)
                *status = RN_JPEG_ST_COEF_LIMIT;
            blk[0] = static_cast<int16_t>(pred);
        } else {
            pred += blk[0];
        }
    }
    return pred;
}

}  // namespace rn_jpeg_huff
