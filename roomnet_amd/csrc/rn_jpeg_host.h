// Host half of the split baseline-JPEG decode: the marker walk (rn_jpeg_probe) and the Huffman pass
// (rn_jpeg_entropy_decode), which is the serial part of a JPEG file.  Everything behind it -- dequantisation, inverse DCT, chroma
// upsampling, colour conversion -- touches every pixel and runs on the GPU (rn_jpeg.hip).  Pure functions on byte buffers: no HIP
// header, no device, no allocation; every read of `data` and every coefficient index is bounded, so arbitrary bytes give RN_OK or
// a negative code and nothing else.  Included by rn_jpeg.hip (which exports the two entry points) and by
// tools/jpeg_corrupt_main.cpp (the host-sanitizer corpus run).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "roomnet_hip.h"

namespace rn_jpeg {

// zigzag position -> natural (row-major) position
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;     // first-level table of the Huffman decoder: codes of up to 9 bits resolve in one lookup

struct HuffTable {
    bool present = false;
    uint8_t bits[17];            // bits[l] = number of codes of length l
    uint8_t vals[256];
    // derived (build_table)
    uint16_t look[1 << kLookBits];   // (length << 8) | symbol of the code that is a prefix of the index; 0 = longer than kLookBits
    int32_t maxcode[18];             // largest code of length l, -1 when there is none; [17] = sentinel
    int32_t valoff[17];              // vals index of the first code of length l minus that code
};

struct Parsed {
    rn_jpeg_info info;
    HuffTable dc[4], ac[4];
    int comp_dc[3], comp_ac[3];
    size_t scan_begin;           // first byte of the entropy-coded segment
};

inline int unsupported(rn_jpeg_info& info, const char* why) {
    if (info.supported) {        // (the first reason stays)
        info.supported = 0;
        std::snprintf(info.reason, sizeof(info.reason), "%s", why);
    }
    return RN_OK;
}

inline bool build_table(HuffTable& t) {
    int code = 0, k = 0;
    std::memset(t.look, 0, sizeof(t.look));
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        if (t.bits[l]) {
            if (code + t.bits[l] > (1 << l)) return false;       // more codes than the length has
            for (int i = 0; i < t.bits[l]; ++i, ++code, ++k) {
                if (l <= kLookBits) {
                    const int first = code << (kLookBits - l);
                    for (int j = 0; j < (1 << (kLookBits - l)); ++j)
                        t.look[first + j] = static_cast<uint16_t>((l << 8) | t.vals[k]);
                }
            }
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    return true;
}

// APP1 "Exif\0\0": IFD0 tag 0x0112 (orientation), either byte order.  Returns the value, 0 when the tag is absent or the segment
// is not readable as TIFF.
inline int exif_orientation(const uint8_t* p, size_t n) {
    if (n < 14 || std::memcmp(p, "Exif\0\0", 6) != 0) return 0;
    const uint8_t* t = p + 6;
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I')
        le = true;
    else if (t[0] == 'M' && t[1] == 'M')
        le = false;
    else
        return 0;
    auto u16 = [&](size_t o) -> uint32_t { return le ? (t[o] | (t[o + 1] << 8)) : ((t[o] << 8) | t[o + 1]); };
    auto u32 = [&](size_t o) -> uint32_t {
        return le ? (u16(o) | (u16(o + 2) << 16)) : ((u16(o) << 16) | u16(o + 2));
    };
    if (u16(2) != 42) return 0;
    const size_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 0;
    const size_t count = u16(ifd);
    for (size_t i = 0; i < count; ++i) {
        const size_t e = ifd + 2 + 12 * i;
        if (e > tn || tn - e < 12) return 0;
        if (u16(e) == 0x0112) return static_cast<int>(u16(e + 8));
    }
    return 0;
}

inline bool contains(const uint8_t* p, size_t n, const char* word) {
    const size_t m = std::strlen(word);
    if (n < m) return false;
    for (size_t i = 0; i + m <= n; ++i)
        if (p[i] == static_cast<uint8_t>(word[0]) && std::memcmp(p + i, word, m) == 0) return true;
    return false;
}

// The marker walk up to the first byte of the scan.  RN_E_INVALID: not a JPEG / truncated or inconsistent headers.
// RN_OK with info.supported = 0 and a reason: a JPEG this decoder leaves to the general one.
inline int parse(const uint8_t* data, size_t len, Parsed& p) {
    rn_jpeg_info& info = p.info;
    std::memset(&info, 0, sizeof(info));
    info.supported = 1;
    for (auto& t : p.dc) t.present = false;
    for (auto& t : p.ac) t.present = false;
    if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return RN_E_INVALID;
    bool have_q[4] = {false, false, false, false}, have_sof = false;
    uint16_t qtab[4][64];
    int comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
    size_t pos = 2;
    for (;;) {
        if (pos >= len || data[pos] != 0xFF) return RN_E_INVALID;
        while (pos < len && data[pos] == 0xFF) ++pos;          // fill bytes
        if (pos >= len) return RN_E_INVALID;
        const int m = data[pos++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;    // TEM, stray RSTn: no payload
        if (m == 0xD8 || m == 0xD9 || m == 0x00) return RN_E_INVALID;      // SOI again / EOI before a scan / stuffed zero
        if (len - pos < 2) return RN_E_INVALID;
        const size_t seg = (static_cast<size_t>(data[pos]) << 8) | data[pos + 1];
        if (seg < 2 || seg > len - pos) return RN_E_INVALID;
        const uint8_t* s = data + pos + 2;
        const size_t n = seg - 2;
        pos += seg;
        if (m == 0xDB) {                                                      // DQT
            size_t o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                ++o;
                if (tq > 3 || pq > 1) return RN_E_INVALID;
                const size_t need = pq ? 128 : 64;
                if (n - o < need) return RN_E_INVALID;
                if (pq) {
                    unsupported(info, "16-bit quantisation table");
                } else {
                    for (int k = 0; k < 64; ++k) qtab[tq][kNatural[k]] = s[o + k];
                    have_q[tq] = true;
                }
                o += need;
            }
        } else if (m == 0xC4) {                                               // DHT
            size_t o = 0;
            while (o < n) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                ++o;
                if (tc > 1 || th > 3 || n - o < 16) return RN_E_INVALID;
                HuffTable& t = tc ? p.ac[th] : p.dc[th];
                size_t total = 0;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) total += (t.bits[l] = s[o + l - 1]);
                o += 16;
                if (total > 256 || n - o < total) return RN_E_INVALID;
                std::memset(t.vals, 0, sizeof(t.vals));
                std::memcpy(t.vals, s + o, total);
                o += total;
                if (!build_table(t)) return RN_E_INVALID;
                t.present = true;
            }
        } else if (m == 0xC0) {                                               // SOF0
            if (have_sof || n < 6) return RN_E_INVALID;
            have_sof = true;
            const int prec = s[0], nc = s[5];
            info.height = (s[1] << 8) | s[2];
            info.width = (s[3] << 8) | s[4];
            if (n < 6 + 3 * static_cast<size_t>(nc) || info.width == 0) return RN_E_INVALID;
            if (prec != 8) return unsupported(info, "not 8-bit");
            if (info.height == 0) return unsupported(info, "height in a DNL segment");
            if (nc != 1 && nc != 3) return unsupported(info, nc == 4 ? "4 components (CMYK / YCCK)" : "component count");
            info.ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = s[6 + 3 * c];
                comp_h[c] = s[7 + 3 * c] >> 4;
                comp_v[c] = s[7 + 3 * c] & 15;
                comp_q[c] = s[8 + 3 * c];
                if (comp_q[c] > 3) return RN_E_INVALID;
            }
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8 && m != 0xCC) {        // the other frame types (0xC4 handled above)
            if (m == 0xC2) return unsupported(info, "progressive");
            if (m >= 0xC9) return unsupported(info, "arithmetic coding");
            return unsupported(info, m == 0xC1 ? "extended sequential" : "lossless / hierarchical");
        } else if (m == 0xCC) {
            return unsupported(info, "arithmetic coding");
        } else if (m == 0xDD) {                                               // DRI
            if (n < 2) return RN_E_INVALID;
            info.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {                                               // APP14
            if (n >= 5 && std::memcmp(s, "Adobe", 5) == 0) unsupported(info, "Adobe APP14 segment");
        } else if (m == 0xE1) {                                               // APP1: EXIF or XMP
            const int o = exif_orientation(s, n);
            if (o >= 2 && o <= 8) unsupported(info, "EXIF orientation is not 1");
            // (an XMP packet can carry tiff:Orientation as well, and the general decoder honours it when EXIF has none)
            if (n >= 4 && std::memcmp(s, "http", 4) == 0 && contains(s, n, "Orientation")) unsupported(info, "XMP orientation");
        } else if (m == 0xDC) {
            unsupported(info, "DNL segment");
        } else if (m == 0xDA) {                                               // SOS
            if (!have_sof || n < 1) return RN_E_INVALID;
            if (!info.supported) return RN_OK;
            const int ns = s[0];
            if (n < 1 + 2 * static_cast<size_t>(ns) + 3) return RN_E_INVALID;
            if (ns != info.ncomp) return unsupported(info, "more than one scan");
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return unsupported(info, "scan order differs from the frame's");
                p.comp_dc[c] = s[2 + 2 * c] >> 4;
                p.comp_ac[c] = s[2 + 2 * c] & 15;
                if (p.comp_dc[c] > 3 || p.comp_ac[c] > 3) return RN_E_INVALID;
                if (!p.dc[p.comp_dc[c]].present || !p.ac[p.comp_ac[c]].present || !have_q[comp_q[c]]) return RN_E_INVALID;
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) return unsupported(info, "not a sequential scan");
            // sampling: grey 1x1; colour with ids 1,2,3, chroma 1x1, luma 1x1 / 2x1 / 2x2
            if (info.ncomp == 1) {
                if (comp_h[0] != 1 || comp_v[0] != 1) return unsupported(info, "grey with sampling factors");
                info.hsamp = info.vsamp = 1;
            } else {
                if (comp_id[0] != 1 || comp_id[1] != 2 || comp_id[2] != 3) return unsupported(info, "component ids are not 1,2,3");
                if (comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return unsupported(info, "chroma sampling");
                info.hsamp = comp_h[0];
                info.vsamp = comp_v[0];
                if (!((info.hsamp == 1 && info.vsamp == 1) || (info.hsamp == 2 && info.vsamp == 1) ||
                      (info.hsamp == 2 && info.vsamp == 2)))
                    return unsupported(info, "luma sampling is not 1x1, 2x1 or 2x2");
            }
            const int mcus_x = (info.width + 8 * info.hsamp - 1) / (8 * info.hsamp);
            const int mcus_y = (info.height + 8 * info.vsamp - 1) / (8 * info.vsamp);
            for (int c = 0; c < info.ncomp; ++c) {
                info.blocks_w[c] = mcus_x * (c == 0 ? info.hsamp : 1);
                info.blocks_h[c] = mcus_y * (c == 0 ? info.vsamp : 1);
                std::memcpy(info.qt[c], qtab[comp_q[c]], sizeof(info.qt[c]));
            }
            p.scan_begin = pos;
            return RN_OK;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

// int16 elements of an image's coefficient buffer: [component][block_y][block_x][64]
inline size_t coeff_count(const rn_jpeg_info& info) {
    size_t n = 0;
    for (int c = 0; c < info.ncomp && c < 3; ++c) n += static_cast<size_t>(info.blocks_w[c]) * info.blocks_h[c] * 64;
    return n;
}

// Entropy-coded bytes -> bits: FF 00 is a stuffed FF; at any other marker, and at the end of the data, the reader stops and
// supplies zero bits, counting them -- a block that consumed one of those is truncated.
struct BitReader {
    const uint8_t* data;
    size_t len, pos;
    uint64_t acc = 0;      // the next bits, left-aligned below bit `cnt`
    int cnt = 0;           // valid bits in acc
    int pad = 0;           // how many of them are made-up zeros (always the last ones)

    inline void fill() {
        while (cnt <= 56) {
            uint32_t b = 0;
            if (pos < len) {
                const uint8_t c = data[pos];
                if (c != 0xFF) {
                    b = c;
                    ++pos;
                } else if (pos + 1 < len && data[pos + 1] == 0x00) {
                    b = 0xFF;
                    pos += 2;
                } else {
                    pad += 8;                  // a marker (or a lone FF at the end): stay in front of it
                }
            } else {
                pad += 8;
            }
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }
    inline uint32_t peek(int n) { return static_cast<uint32_t>(acc >> (cnt - n)) & ((1u << n) - 1u); }   // 1 <= n <= 16, cnt >= n
    inline void skip(int n) { cnt -= n; }
    inline bool overrun() const { return cnt < pad; }
    inline void reset() { acc = 0; cnt = 0; pad = 0; }
};

// one Huffman symbol, or -1 for a code the table does not have
inline int decode_symbol(BitReader& br, const HuffTable& t) {
    if (br.cnt < 16) br.fill();
    const uint16_t e = t.look[br.peek(kLookBits)];
    if (e) {
        br.skip(e >> 8);
        return e & 0xFF;
    }
    int l = kLookBits + 1;
    int32_t code = static_cast<int32_t>(br.peek(l));
    while (l <= 16 && code > t.maxcode[l]) {
        ++l;
        if (l <= 16) code = static_cast<int32_t>(br.peek(l));
    }
    if (l > 16) return -1;
    br.skip(l);
    const int idx = code + t.valoff[l];
    if (idx < 0 || idx > 255) return -1;
    return t.vals[idx];
}

// the s-bit magnitude field as a signed value (JPEG's EXTEND)
inline int receive_extend(BitReader& br, int s) {
    if (br.cnt < s) br.fill();
    const int v = static_cast<int>(br.peek(s));
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// The Huffman pass.  `info` must be what rn_jpeg_probe returned for these bytes (the headers are walked again here: the
// Huffman tables are not part of rn_jpeg_info, and the sizes every index is bounded by are taken from THESE bytes).
// coeffs [component][block_y][block_x][64] natural order, `cap` int16 elements available.
inline int entropy_decode(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap, const char** why) {
    static thread_local Parsed p;      // 12 KB of tables: not on the stack of a pool thread, not allocated per image
    *why = "";
    if (!info || !coeffs) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    if (parse(data, len, p) != RN_OK) {
        *why = "not a JPEG file, or its headers are truncated";
        return RN_E_INVALID;
    }
    if (!p.info.supported) {
        *why = "unsupported file";
        return RN_E_INVALID;
    }
    const rn_jpeg_info& pi = p.info;
    if (info->width != pi.width || info->height != pi.height || info->ncomp != pi.ncomp || info->hsamp != pi.hsamp ||
        info->vsamp != pi.vsamp) {
        *why = "the info does not describe these bytes";
        return RN_E_INVALID;
    }
    const size_t total = coeff_count(pi);
    if (total > cap) {
        *why = "coefficient buffer too small";
        return RN_E_RANGE;
    }
    int16_t* base[3];
    size_t off = 0;
    for (int c = 0; c < pi.ncomp; ++c) {
        base[c] = coeffs + off;
        off += static_cast<size_t>(pi.blocks_w[c]) * pi.blocks_h[c] * 64;
    }
    const int mcus_x = pi.blocks_w[0] / pi.hsamp, mcus_y = pi.blocks_h[0] / pi.vsamp;
    BitReader br{data, len, p.scan_begin};
    int pred[3] = {0, 0, 0};
    int until_restart = pi.restart_interval, next_rst = 0;
    for (int my = 0; my < mcus_y; ++my) {
        for (int mx = 0; mx < mcus_x; ++mx) {
            if (pi.restart_interval && until_restart == 0) {
                // byte-align (the bits left are padding), then the marker FF Dn with n counting mod 8
                if (br.overrun()) {
                    *why = "scan data truncated";
                    return RN_E_INVALID;
                }
                br.reset();
                size_t q = br.pos;
                while (q < len && data[q] == 0xFF) ++q;
                if (q >= len || q == br.pos || data[q] != 0xD0 + next_rst) {
                    *why = "restart marker missing";
                    return RN_E_INVALID;
                }
                br.pos = q + 1;
                next_rst = (next_rst + 1) & 7;
                until_restart = pi.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < pi.ncomp; ++c) {
                const int hs = c == 0 ? pi.hsamp : 1, vs = c == 0 ? pi.vsamp : 1;
                const HuffTable& dct = p.dc[p.comp_dc[c]];
                const HuffTable& act = p.ac[p.comp_ac[c]];
                const uint16_t* qt = pi.qt[c];
                for (int v = 0; v < vs; ++v)
                    for (int hh = 0; hh < hs; ++hh) {
                        const size_t by = static_cast<size_t>(my) * vs + v, bx = static_cast<size_t>(mx) * hs + hh;
                        int16_t* blk = base[c] + (by * pi.blocks_w[c] + bx) * 64;      // by < blocks_h, bx < blocks_w by construction
                        std::memset(blk, 0, 128);
                        int s = decode_symbol(br, dct);
                        if (s < 0 || s > 15) {
                            *why = "invalid DC code";
                            return RN_E_INVALID;
                        }
                        if (s) pred[c] += receive_extend(br, s);
                        // |pred| itself stays within the limit (a table entry may be 0), so the sum above cannot overflow
                        const int dc = pred[c] * static_cast<int>(qt[0]);
                        if (pred[c] > RN_JPEG_COEF_LIMIT || pred[c] < -RN_JPEG_COEF_LIMIT || dc > RN_JPEG_COEF_LIMIT ||
                            dc < -RN_JPEG_COEF_LIMIT) {
                            *why = "dequantised coefficient beyond RN_JPEG_COEF_LIMIT";
                            return RN_E_INVALID;
                        }
                        blk[0] = static_cast<int16_t>(pred[c]);
                        for (int k = 1; k < 64; ++k) {
                            const int rs = decode_symbol(br, act);
                            if (rs < 0) {
                                *why = "invalid AC code";
                                return RN_E_INVALID;
                            }
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;          // EOB
                                k += 15;                     // ZRL
                                continue;
                            }
                            k += r;
                            if (k > 63) {
                                *why = "AC run past the block";
                                return RN_E_INVALID;
                            }
                            const int val = receive_extend(br, s);       // |val| < 2^15
                            const int nat = kNatural[k];
                            const int dq = val * static_cast<int>(qt[nat]);       // < 2^15 * 2^8
                            if (dq > RN_JPEG_COEF_LIMIT || dq < -RN_JPEG_COEF_LIMIT) {
                                *why = "dequantised coefficient beyond RN_JPEG_COEF_LIMIT";
                                return RN_E_INVALID;
                            }
                            blk[nat] = static_cast<int16_t>(val);
                        }
                        if (br.overrun()) {
                            *why = "scan data truncated";
                            return RN_E_INVALID;
                        }
                    }
            }
            --until_restart;
        }
    }
    return RN_OK;
}

}  // namespace rn_jpeg
