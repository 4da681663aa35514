// Host side of the parallel Huffman decode: rn_jpeg_scan_probe's body, and the HOST MODEL of the four
// phases rn_jpeg_huff.hip launches -- the same lanes through the same rn_jpeg_huff.h, run one after another, the same status codes.
// Pure functions on byte buffers like rn_jpeg_host.h: no HIP header, no device.  Included by rn_jpeg_huff.hip (which exports
// rn_jpeg_scan_probe and rn_jpeg_huffman_model) and by tools/jpeg_huff_model_main.cpp (the host-sanitizer corpus run).
#pragma once
#include <vector>

#include "rn_jpeg_host.h"
#include "rn_jpeg_huff.h"

namespace rn_jpeg_huff {

inline void copy_table(const rn_jpeg::HuffTable& from, rn_jpeg_hufftab& to) {
    static_assert(sizeof(to.look) == sizeof(from.look) && sizeof(to.maxcode) == sizeof(from.maxcode) &&
                  sizeof(to.valoff) == sizeof(from.valoff) && sizeof(to.vals) == sizeof(from.vals), "the same tables");
    std::memcpy(to.look, from.look, sizeof(to.look));
    std::memcpy(to.maxcode, from.maxcode, sizeof(to.maxcode));
    std::memcpy(to.valoff, from.valoff, sizeof(to.valoff));
    to.valoff[0] = 0;                                           // (build_table leaves entry 0 unset; nothing reads it)
    std::memcpy(to.vals, from.vals, sizeof(to.vals));
}

// the scan of a parsed, supported file: its byte range (to the end of the data: the decoders find the marker that ends it) and the
// components' tables
inline void fill_scan(const rn_jpeg::Parsed& p, size_t len, rn_jpeg_scan* out) {
    std::memset(out, 0, sizeof(*out));
    out->scan_begin = p.scan_begin;
    out->scan_len = len - p.scan_begin;
    for (int c = 0; c < p.info.ncomp; ++c) {
        copy_table(p.dc[p.comp_dc[c]], out->dc[c]);
        copy_table(p.ac[p.comp_ac[c]], out->ac[c]);
    }
}

inline int scan_probe(const uint8_t* data, size_t len, rn_jpeg_scan* out, bool oriented = false) {
    static thread_local rn_jpeg::Parsed p;
    std::memset(out, 0, sizeof(*out));
    const int rc = rn_jpeg::parse(data, len, p, oriented);
    if (rc != RN_OK) return rc;
    if (p.info.supported) fill_scan(p, len, out);
    return RN_OK;
}

inline void fill_tables(const rn_jpeg_scan& scan, const rn_jpeg_info& info, Tables* t) {
    std::memcpy(t->dc, scan.dc, sizeof(t->dc));
    std::memcpy(t->ac, scan.ac, sizeof(t->ac));
    std::memcpy(t->qt, info.qt, sizeof(t->qt));
    std::memcpy(t->natural, rn_jpeg::kNatural, sizeof(t->natural));
}

struct ModelRounds {
    int inside = 0;      // most rounds a group took in phase 2
    int across = 0;      // rounds of the launch across groups
};

// The four phases on a scan whose headers were parsed.  coef: rn_jpeg::coeff_count(info) elements.
inline int32_t model_scan(const uint8_t* scan, uint32_t scan_len, const rn_jpeg_info& info, const Tables& tables, int16_t* coef,
                          uint32_t subseq_bytes, ModelRounds* rounds) {
    int32_t status = precheck(scan_len);
    if (status != RN_JPEG_ST_OK) return status;
    Ctx c{scan, scan_len, &tables, geometry(info)};
    const uint32_t nsub = subseq_count(scan_len, subseq_bytes);
    std::vector<State> exit_state(nsub);
    NoSink none;
    // 1: speculate
    for (uint32_t i = 0; i < nsub; ++i)
        exit_state[i] = decode_subsequence(c, guess(scan, scan_len, subseq_bytes, i), subseq_end_bit(scan_len, subseq_bytes, i), none);
    // 2a: inside groups, every lane from its left neighbour's stored state, until a round changes nothing
    const uint32_t ngroups = (nsub + kGroup - 1) / kGroup;
    std::vector<State> next(kGroup);
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t first = g * kGroup, count = nsub - first < static_cast<uint32_t>(kGroup) ? nsub - first : kGroup;
        std::vector<State> last_in(count, State{0, kInvalid, 0, 1});     // (pad 1: no entry state yet)
        for (uint32_t round = 1; round < count; ++round) {
            bool changed = false;
            for (uint32_t t = 1; t < count; ++t) {
                const State in = entry_of(exit_state[first + t - 1]);
                next[t] = exit_state[first + t];
                if (last_in[t].pad || in.p != last_in[t].p || in.sk != last_in[t].sk) {      // (the same entry gives the same exit)
                    next[t] = decode_subsequence(c, in, subseq_end_bit(scan_len, subseq_bytes, first + t), none);
                    last_in[t] = in;
                }
                changed |= !same(next[t], exit_state[first + t]);
            }
            if (!changed) break;
            for (uint32_t t = 1; t < count; ++t) exit_state[first + t] = next[t];
            if (rounds && static_cast<int>(round) > rounds->inside) rounds->inside = static_cast<int>(round);
        }
    }
    // 2b: across groups, one walker per group from the last state of the group in front, until it meets what is stored
    for (uint32_t round = 1; round < ngroups; ++round) {
        bool changed = false;
        std::vector<State> in(ngroups);
        for (uint32_t g = 1; g < ngroups; ++g) in[g] = exit_state[g * kGroup - 1];
        for (uint32_t g = 1; g < ngroups; ++g) {
            State s = in[g];
            for (uint32_t j = g * kGroup; j < nsub && j < (g + 1) * kGroup; ++j) {
                const State out = decode_subsequence(c, entry_of(s), subseq_end_bit(scan_len, subseq_bytes, j), none);
                if (same(out, exit_state[j])) break;
                exit_state[j] = out;
                changed = true;
                s = out;
            }
        }
        if (!changed) break;
        if (rounds) rounds->across = static_cast<int>(round);
    }
    // 3: zero, exclusive scan of the block counts, write
    const size_t count = rn_jpeg::coeff_count(info);
    std::memset(coef, 0, count * sizeof(int16_t));
    std::vector<uint32_t> base(nsub);
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        base[i] = blocks;
        blocks += exit_state[i].n;
    }
    int16_t* comp_base[3] = {coef, coef, coef};
    size_t off = 0;
    for (int k = 0; k < info.ncomp; ++k) {
        comp_base[k] = coef + off;
        off += static_cast<size_t>(info.blocks_w[k]) * info.blocks_h[k] * 64;
    }
    for (uint32_t i = 0; i < nsub; ++i) {
        Writer w{&c.g, &tables, {comp_base[0], comp_base[1], comp_base[2]}, base[i]};
        const State entry = i == 0 ? guess(scan, scan_len, subseq_bytes, 0) : entry_of(exit_state[i - 1]);
        const int32_t s = write_lane(c, entry, exit_state[i], subseq_end_bit(scan_len, subseq_bytes, i), i + 1 == nsub, w);
        if (s > status) status = s;
    }
    // 4: DC prediction per component
    for (int k = 0; k < info.ncomp; ++k) {
        int32_t s = RN_JPEG_ST_OK;
        dc_run(c.g, k, 0, static_cast<uint32_t>(info.blocks_w[k]) * info.blocks_h[k], 0, info.qt[k][0], comp_base[k], &s, nullptr);
        if (s > status) status = s;
    }
    return status;
}

// rn_jpeg_huffman_model: arguments as rn_jpeg_entropy_decode takes them, refused the same way
inline int model(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap, int subseq_bytes,
                 int32_t* status, ModelRounds* rounds, const char** why) {
    static thread_local rn_jpeg::Parsed p;
    static thread_local rn_jpeg_scan scan;
    static thread_local Tables tables;
    *why = "";
    if (!info || !coeffs || !status) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    if (subseq_bytes < 4 || subseq_bytes > 4096) {
        *why = "subseq_bytes outside 4 .. 4096";
        return RN_E_RANGE;
    }
    if (rn_jpeg::parse(data, len, p, rn_jpeg::turned(*info)) != RN_OK) {
        *why = "not a JPEG file, or its headers are truncated";
        return RN_E_INVALID;
    }
    if (!p.info.supported) {
        *why = "unsupported file";
        return RN_E_INVALID;
    }
    const rn_jpeg_info& pi = p.info;
    if (!rn_jpeg::describes(*info, pi)) {
        *why = "the info does not describe these bytes";
        return RN_E_INVALID;
    }
    if (rn_jpeg::coeff_count(pi) > cap) {
        *why = "coefficient buffer too small";
        return RN_E_RANGE;
    }
    fill_scan(p, len, &scan);
    fill_tables(scan, pi, &tables);
    if (scan.scan_len > kMaxScanBytes) {
        *status = RN_JPEG_ST_TOO_LARGE;
        return RN_OK;
    }
    *status = model_scan(data + scan.scan_begin, static_cast<uint32_t>(scan.scan_len), pi, tables, coeffs,
                         static_cast<uint32_t>(subseq_bytes), rounds);
    return RN_OK;
}

}  // namespace rn_jpeg_huff
