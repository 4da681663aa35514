// Host half of the split baseline-JPEG decode: the marker walk (rn_jpeg_probe) and the Huffman pass
// (rn_jpeg_entropy_decode), which is the serial part of a JPEG file.  Everything behind it -- dequantisation, inverse DCT, chroma
// upsampling, colour conversion -- touches every pixel and runs on the GPU (rn_jpeg.hip).  Pure functions on byte buffers: no HIP
// header, no device, no allocation; every read of `data` and every coefficient index is bounded, so arbitrary bytes give RN_OK or
// a negative code and nothing else.  Included by rn_jpeg.hip (which exports the two entry points) and by
// tools/jpeg_corrupt_main.cpp (the host-sanitizer corpus run).
// Further down, the host half of the split ENCODE: the description of the output file
// (rn_jpeg_encode_info) and its Huffman pass (rn_jpeg_entropy_encode), with the same properties; exported by rn_jpeg_enc.hip and
// run stand-alone by tools/jpeg_encode_main.cpp.  rn_jpeg_huffenc.h restates the pass per zigzag position for the GPU (DESIGN.md
// section 19) on the tables, the header writer and the ByteWriter of this file.
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
    int orient;                  // oriented walk: the EXIF orientation the first Exif segment gives, 1..8
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
// is not readable as TIFF.  *plain (when asked for): false for an entry that is not one SHORT, the only form the oriented walk takes.
inline int exif_orientation(const uint8_t* p, size_t n, bool* plain = nullptr) {
    if (plain) *plain = true;
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
        if (u16(e) == 0x0112) {
            if (plain) *plain = u16(e + 2) == 3 && u32(e + 4) == 1;
            return static_cast<int>(u16(e + 8));
        }
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
// `oriented` (rn_jpeg_probe_oriented): an EXIF orientation of 2..8 is no refusal; the file's info.supported
// becomes that orientation.  The first Exif segment decides, as it does for Pillow; a tag value outside 2..8 reads as 1; a later
// Exif segment that reads otherwise, and an orientation entry that is not one SHORT, are refusals.  Everything else is the same walk.
inline int parse(const uint8_t* data, size_t len, Parsed& p, bool oriented = false) {
    rn_jpeg_info& info = p.info;
    std::memset(&info, 0, sizeof(info));
    info.supported = 1;
    p.orient = 1;
    bool have_exif = false;
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
            if (!oriented) {
                const int o = exif_orientation(s, n);
                if (o >= 2 && o <= 8) unsupported(info, "EXIF orientation is not 1");
            } else if (n >= 6 && std::memcmp(s, "Exif\0\0", 6) == 0) {
                bool plain = true;
                const int o = exif_orientation(s, n, &plain);
                const int reading = o >= 2 && o <= 8 ? o : 1;
                if (!plain) {
                    unsupported(info, "EXIF orientation entry is not one SHORT");
                } else if (!have_exif) {
                    have_exif = true;
                    p.orient = reading;
                } else if (reading != p.orient) {
                    unsupported(info, "conflicting EXIF segments");
                }
            }
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
            info.supported = p.orient;       // (1 unless the walk is the oriented one)
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

// info.supported of a file the oriented walk took: the EXIF orientation the pixels are to be turned by
inline bool turned(const rn_jpeg_info& info) { return info.supported >= 2 && info.supported <= 8; }

// what a second walk of the bytes must find again for `info` to describe them; the orientation too when the info carries one
inline bool describes(const rn_jpeg_info& info, const rn_jpeg_info& pi) {
    return info.width == pi.width && info.height == pi.height && info.ncomp == pi.ncomp && info.hsamp == pi.hsamp &&
           info.vsamp == pi.vsamp && (!turned(info) || info.supported == pi.supported);
}

// The Huffman pass.  `info` must be what rn_jpeg_probe (or rn_jpeg_probe_oriented: the walk is then the oriented one) returned for
// these bytes (the headers are walked again here: the Huffman tables are not part of rn_jpeg_info, and the sizes every index is
// bounded by are taken from THESE bytes).
// coeffs [component][block_y][block_x][64] natural order, `cap` int16 elements available.
inline int entropy_decode(const uint8_t* data, size_t len, const rn_jpeg_info* info, int16_t* coeffs, size_t cap, const char** why) {
    static thread_local Parsed p;      // 12 KB of tables: not on the stack of a pool thread, not allocated per image
    *why = "";
    if (!info || !coeffs) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    if (parse(data, len, p, turned(*info)) != RN_OK) {
        *why = "not a JPEG file, or its headers are truncated";
        return RN_E_INVALID;
    }
    if (!p.info.supported) {
        *why = "unsupported file";
        return RN_E_INVALID;
    }
    const rn_jpeg_info& pi = p.info;
    if (!describes(*info, pi)) {
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

// ---- the encoder's host half: the decode above, mirrored -----------------------------------------------
// rn_jpeg_encode_info describes the file imwrite writes for a .jpg name (4:2:0, libjpeg's quality scaling of the standard
// tables), the GPU turns pixels into the quantised coefficients of that file (rn_jpeg_enc.hip), and entropy_encode writes the
// file: its headers, the Huffman pass with the standard tables of JPEG Annex K, EOI.  Same properties as the decoder: no device,
// no allocation, every write of `out` bounded by `cap`.

// Annex K.1 in natural order
static const uint8_t kStdLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                      14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kStdChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: code counts per length 1..16, then the symbols in code order
static const uint8_t kStdDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kStdAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kStdAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// libjpeg's jpeg_set_quality: the standard tables scaled by 5000 / q below 50, else 200 - 2 q; entries clamped to 1..255
inline void quality_table(const uint8_t (&std_table)[64], int quality, uint16_t* out) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int v = (std_table[k] * scale + 50) / 100;
        out[k] = static_cast<uint16_t>(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

inline int encode_info(int width, int height, int quality, rn_jpeg_info* out) {
    if (!out || quality < 1 || quality > 100 || width < 1 || height < 1 || width > 65535 || height > 65535) return RN_E_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->width = width;
    out->height = height;
    out->ncomp = 3;
    out->hsamp = out->vsamp = 2;
    const int mcus_x = (width + 15) / 16, mcus_y = (height + 15) / 16;
    for (int c = 0; c < 3; ++c) {
        out->blocks_w[c] = mcus_x * (c == 0 ? 2 : 1);
        out->blocks_h[c] = mcus_y * (c == 0 ? 2 : 1);
    }
    quality_table(kStdLumaQ, quality, out->qt[0]);
    quality_table(kStdChromaQ, quality, out->qt[1]);
    std::memcpy(out->qt[2], out->qt[1], sizeof(out->qt[2]));
    out->supported = 1;
    return RN_OK;
}

// an info as encode_info fills it (whatever the quality was): the only kind of file the encoder writes
inline bool encode_info_ok(const rn_jpeg_info& f) {
    if (f.supported != 1 || f.ncomp != 3 || f.hsamp != 2 || f.vsamp != 2 || f.restart_interval != 0) return false;
    if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535) return false;
    const int mcus_x = (f.width + 15) / 16, mcus_y = (f.height + 15) / 16;
    for (int c = 0; c < 3; ++c)
        if (f.blocks_w[c] != mcus_x * (c == 0 ? 2 : 1) || f.blocks_h[c] != mcus_y * (c == 0 ? 2 : 1)) return false;
    for (int k = 0; k < 64; ++k) {
        if (f.qt[0][k] < 1 || f.qt[0][k] > 255 || f.qt[1][k] < 1 || f.qt[1][k] > 255) return false;
        if (f.qt[2][k] != f.qt[1][k]) return false;       // (Cb and Cr share table 1 of the file)
    }
    return true;
}

constexpr size_t kEncHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 14;      // SOI .. SOS, as entropy_encode writes them
// Worst case of one block: a DC code of at most 9 bits + 11 magnitude bits, 63 AC codes of at most 16 + 10 bits = 1658 bits,
// every byte of them FF and stuffed.
constexpr size_t kEncBlockBytes = 2 * ((9 + 11 + 63 * 26 + 7) / 8);

inline size_t encoded_bound(const rn_jpeg_info& f) {
    return kEncHeaderBytes + (coeff_count(f) / 64) * kEncBlockBytes + 2 /* padding byte, stuffed */ + 2 /* EOI */;
}

struct EncTable {
    uint16_t code[256];
    uint8_t size[256];       // 0: the table has no code for the symbol
};

inline void build_enc_table(const uint8_t* bits, const uint8_t* vals, EncTable& t) {
    std::memset(&t, 0, sizeof(t));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++code, ++k) {
            t.code[vals[k]] = static_cast<uint16_t>(code);
            t.size[vals[k]] = static_cast<uint8_t>(l);
        }
        code <<= 1;
    }
}

// Bytes into out[0 .. cap): past cap nothing is stored, the count goes on (the caller learns the size it needed).
struct ByteWriter {
    uint8_t* out;
    size_t cap, pos = 0;
    uint64_t acc = 0;        // pending bits, right-aligned
    int cnt = 0;
    inline void byte(uint32_t b) {
        if (pos < cap) out[pos] = static_cast<uint8_t>(b);
        ++pos;
    }
    inline void u16(uint32_t v) {
        byte(v >> 8);
        byte(v & 255);
    }
    inline void bits(uint32_t v, int n) {       // n <= 26, v < 2^n
        acc = (acc << n) | v;
        cnt += n;
        while (cnt >= 8) {
            const uint32_t b = static_cast<uint32_t>(acc >> (cnt - 8)) & 255u;
            byte(b);
            if (b == 0xFF) byte(0);
            cnt -= 8;
        }
    }
    inline void flush() {                       // the last byte is padded with 1-bits
        if (cnt) bits((1u << (8 - cnt)) - 1u, 8 - cnt);
    }
};

// SOI .. SOS of the file of `f` (an info encode_info fills): kEncHeaderBytes bytes.  The one place the header is written:
// entropy_encode and rn_jpeg_encode_headers (rn_jpeg_huffenc.h) both call it.
inline void write_headers(const rn_jpeg_info& f, ByteWriter& w) {
    w.u16(0xFFD8);
    w.u16(0xFFE0);                                           // APP0: JFIF 1.01, no units, 1:1, no thumbnail
    w.u16(16);
    for (const uint8_t b : {0x4A, 0x46, 0x49, 0x46, 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00}) w.byte(b);
    for (int t = 0; t < 2; ++t) {                            // DQT, zigzag order
        w.u16(0xFFDB);
        w.u16(67);
        w.byte(t);
        for (int k = 0; k < 64; ++k) w.byte(f.qt[t][kNatural[k]]);
    }
    w.u16(0xFFC0);                                           // SOF0
    w.u16(17);
    w.byte(8);
    w.u16(static_cast<uint32_t>(f.height));
    w.u16(static_cast<uint32_t>(f.width));
    w.byte(3);
    for (const uint8_t b : {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) w.byte(b);
    for (int t = 0; t < 2; ++t)                              // DHT: DC0, AC0, DC1, AC1
        for (int cls = 0; cls < 2; ++cls) {
            const uint8_t* bits = cls ? kStdAcBits[t] : kStdDcBits[t];
            const uint8_t* vals = cls ? kStdAcVals[t] : kStdDcVals;
            const int count = cls ? 162 : 12;
            w.u16(0xFFC4);
            w.u16(static_cast<uint32_t>(2 + 1 + 16 + count));
            w.byte(static_cast<uint32_t>((cls << 4) | t));
            for (int l = 0; l < 16; ++l) w.byte(bits[l]);
            for (int k = 0; k < count; ++k) w.byte(vals[k]);
        }
    w.u16(0xFFDA);                                           // SOS: one interleaved scan
    w.u16(12);
    for (const uint8_t b : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) w.byte(b);
}

inline int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// The whole file for the quantised coefficients `coeffs` ([component][block_y][block_x][64], natural order: the layout
// entropy_decode writes).  *len: the file's size, also when it is more than cap (RN_E_RANGE; out[0 .. cap) is then its beginning).
inline int entropy_encode(const rn_jpeg_info* info, const int16_t* coeffs, uint8_t* out, size_t cap, size_t* len, const char** why) {
    static thread_local EncTable dc[2], ac[2];
    static thread_local bool built = false;
    *why = "";
    if (!info || !coeffs || !len || (!out && cap)) {
        *why = "null argument";
        return RN_E_INVALID;
    }
    *len = 0;
    if (!encode_info_ok(*info)) {
        *why = "the info is not one rn_jpeg_encode_info fills (3 components, 4:2:0, whole-MCU grids, 8-bit tables)";
        return RN_E_INVALID;
    }
    if (!built) {
        for (int t = 0; t < 2; ++t) {
            build_enc_table(kStdDcBits[t], kStdDcVals, dc[t]);
            build_enc_table(kStdAcBits[t], kStdAcVals[t], ac[t]);
        }
        built = true;
    }
    const rn_jpeg_info& f = *info;
    ByteWriter w{out, cap};
    write_headers(f, w);

    const int16_t* base[3];
    size_t off = 0;
    for (int c = 0; c < 3; ++c) {
        base[c] = coeffs + off;
        off += static_cast<size_t>(f.blocks_w[c]) * f.blocks_h[c] * 64;
    }
    const int mcus_x = f.blocks_w[1], mcus_y = f.blocks_h[1];
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < mcus_y; ++my)
        for (int mx = 0; mx < mcus_x; ++mx)
            for (int c = 0; c < 3; ++c) {
                const int s = c == 0 ? 2 : 1;
                const EncTable& dct = dc[c ? 1 : 0];
                const EncTable& act = ac[c ? 1 : 0];
                for (int v = 0; v < s; ++v)
                    for (int hh = 0; hh < s; ++hh) {
                        const size_t by = static_cast<size_t>(my) * s + v, bx = static_cast<size_t>(mx) * s + hh;
                        const int16_t* blk = base[c] + (by * f.blocks_w[c] + bx) * 64;
                        // encode_one_block of jchuff.c
                        const int diff = blk[0] - pred[c];
                        pred[c] = blk[0];
                        int nbits = bit_length(static_cast<uint32_t>(diff < 0 ? -diff : diff));
                        if (nbits > 11) {
                            *why = "DC difference beyond category 11";
                            return RN_E_INVALID;
                        }
                        w.bits(dct.code[nbits], dct.size[nbits]);
                        if (nbits) w.bits(static_cast<uint32_t>(diff < 0 ? diff - 1 : diff) & ((1u << nbits) - 1u), nbits);
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            const int val = blk[kNatural[k]];
                            if (val == 0) {
                                ++run;
                                continue;
                            }
                            while (run > 15) {
                                w.bits(act.code[0xF0], act.size[0xF0]);      // ZRL
                                run -= 16;
                            }
                            nbits = bit_length(static_cast<uint32_t>(val < 0 ? -val : val));
                            if (nbits > 10) {
                                *why = "AC coefficient beyond category 10";
                                return RN_E_INVALID;
                            }
                            const int sym = (run << 4) | nbits;
                            w.bits(act.code[sym], act.size[sym]);
                            w.bits(static_cast<uint32_t>(val < 0 ? val - 1 : val) & ((1u << nbits) - 1u), nbits);
                            run = 0;
                        }
                        if (run > 0) w.bits(act.code[0x00], act.size[0x00]);      // EOB
                    }
            }
    w.flush();
    w.u16(0xFFD9);
    *len = w.pos;
    if (w.pos > cap) {
        *why = "output buffer too small";
        return RN_E_RANGE;
    }
    return RN_OK;
}

}  // namespace rn_jpeg
