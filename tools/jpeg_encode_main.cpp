// Host-sanitizer run of the JPEG entropy encoder (roomnet_amd/csrc/rn_jpeg_host.h): a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/jpeg_encode_main.cpp -o build/jpeg_encode && build/jpeg_encode
//
// For several sizes (one block, odd sizes, sizes that are no multiple of the MCU, more than one MCU row) seeded random in-range
// coefficient arrays -- sparse, dense, long zero runs -- are encoded twice: once to learn the length, then into a heap block of
// EXACTLY that many bytes, so AddressSanitizer sees any write past it; the file is decoded back with rn_jpeg::entropy_decode and
// compared.  Then the refusals: a cap one byte short and a cap of zero (RN_E_RANGE), coefficients beyond the Huffman categories,
// infos the encoder does not write (RN_E_INVALID).  Prints one summary line; exit status 0 unless something differed
// (sanitizer findings abort the run themselves).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rn_jpeg_host.h"

namespace {

uint64_t g_seed = 0x9e3779b97f4a7c15ull;
uint64_t next() {
    g_seed ^= g_seed << 13;
    g_seed ^= g_seed >> 7;
    g_seed ^= g_seed << 17;
    return g_seed;
}
int in_range(int lim) { return static_cast<int>(next() % (2 * lim + 1)) - lim; }      // -lim .. lim

// DC values within +-1023 (differences within category 11), AC values within category 10
void fill(std::vector<int16_t>& c, int mode) {
    for (size_t b = 0; b < c.size() / 64; ++b) {
        int16_t* blk = c.data() + b * 64;
        blk[0] = static_cast<int16_t>(in_range(1023));
        for (int k = 1; k < 64; ++k) {
            const bool zero = mode == 0 ? next() % 5 != 0 : (mode == 1 ? false : k != 63 && k != 17);
            blk[k] = zero ? 0 : static_cast<int16_t>(in_range(1023));
        }
    }
}

int check(bool ok, const char* what, int w, int h) {
    if (!ok) std::printf("FAILED: %s (%dx%d)\n", what, w, h);
    return ok ? 0 : 1;
}

int run_size(int w, int h, int quality, long& files) {
    rn_jpeg_info info;
    int bad = check(rn_jpeg::encode_info(w, h, quality, &info) == RN_OK, "encode_info", w, h);
    if (bad) return bad;
    const size_t count = rn_jpeg::coeff_count(info);
    std::vector<int16_t> c(count);
    const char* why = "";
    for (int mode = 0; mode < 3; ++mode) {
        fill(c, mode);
        size_t len = 0, len2 = 0;
        // exact-size heap copies of the input too: a read past the coefficients is seen as well
        int16_t* coeffs = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t)));
        std::memcpy(coeffs, c.data(), count * sizeof(int16_t));
        bad |= check(rn_jpeg::entropy_encode(&info, coeffs, nullptr, 0, &len, &why) == RN_E_RANGE && len > rn_jpeg::kEncHeaderBytes,
                     "cap 0 is RN_E_RANGE with the length", w, h);
        bad |= check(len <= rn_jpeg::encoded_bound(info), "the length is within encoded_bound", w, h);
        uint8_t* out = static_cast<uint8_t*>(std::malloc(len));
        bad |= check(rn_jpeg::entropy_encode(&info, coeffs, out, len, &len2, &why) == RN_OK && len2 == len, "encode into exactly len bytes", w, h);
        uint8_t* shorter = static_cast<uint8_t*>(std::malloc(len - 1));
        bad |= check(rn_jpeg::entropy_encode(&info, coeffs, shorter, len - 1, &len2, &why) == RN_E_RANGE && len2 == len &&
                         std::memcmp(shorter, out, len - 1) == 0,
                     "cap len - 1 is RN_E_RANGE", w, h);
        std::free(shorter);
        static rn_jpeg::Parsed p;
        bad |= check(rn_jpeg::parse(out, len, p) == RN_OK && p.info.supported == 1 && p.info.width == w && p.info.height == h &&
                         std::memcmp(p.info.qt, info.qt, sizeof(info.qt)) == 0 && rn_jpeg::coeff_count(p.info) == count,
                     "the file's headers describe the info", w, h);
        int16_t* back = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t)));
        const rn_jpeg_info parsed = p.info;
        // (the decoder refuses |coef * q| > RN_JPEG_COEF_LIMIT, which random values at a low quality exceed: quality 100 has q = 1)
        const int rc = rn_jpeg::entropy_decode(out, len, &parsed, back, count, &why);
        bad |= check(rc == RN_OK && std::memcmp(back, coeffs, count * sizeof(int16_t)) == 0, "decode(encode(c)) == c", w, h);
        std::free(back);
        std::free(out);
        std::free(coeffs);
        ++files;
    }
    // out of range values
    std::vector<uint8_t> buf(rn_jpeg::encoded_bound(info));
    size_t len = 0;
    std::fill(c.begin(), c.end(), static_cast<int16_t>(0));
    c[9] = 1024;
    bad |= check(rn_jpeg::entropy_encode(&info, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "AC 1024 is RN_E_INVALID", w, h);
    c[9] = -32768;
    bad |= check(rn_jpeg::entropy_encode(&info, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "AC -32768 is RN_E_INVALID", w, h);
    c[9] = 0;
    c[0] = 2048;
    bad |= check(rn_jpeg::entropy_encode(&info, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "DC difference 2048 is RN_E_INVALID", w, h);
    c[0] = 32767;
    c[64] = -32768;
    bad |= check(rn_jpeg::entropy_encode(&info, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "DC difference 65535 is RN_E_INVALID", w, h);
    c[0] = c[64] = 0;
    // infos the encoder does not write
    rn_jpeg_info other = info;
    other.ncomp = 1;
    other.hsamp = other.vsamp = 1;
    bad |= check(rn_jpeg::entropy_encode(&other, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "grey is RN_E_INVALID", w, h);
    other = info;
    other.vsamp = 1;
    bad |= check(rn_jpeg::entropy_encode(&other, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "4:2:2 is RN_E_INVALID", w, h);
    other = info;
    other.blocks_h[2] += 1;
    bad |= check(rn_jpeg::entropy_encode(&other, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "an inconsistent grid is RN_E_INVALID", w, h);
    other = info;
    other.supported = 0;
    bad |= check(rn_jpeg::entropy_encode(&other, c.data(), buf.data(), buf.size(), &len, &why) == RN_E_INVALID, "supported = 0 is RN_E_INVALID", w, h);
    return bad;
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {8, 8}, {16, 16}, {17, 33}, {53, 37}, {2, 31}, {49, 50}, {96, 72}, {200, 120}, {320, 240}};
    int bad = 0;
    long files = 0;
    for (const auto& s : sizes) bad |= run_size(s[0], s[1], 100, files);
    rn_jpeg_info info;
    const int refused[][3] = {{0, 1, 95}, {1, 0, 95}, {65536, 1, 95}, {1, 65536, 95}, {1, 1, 0}, {1, 1, 101}};
    for (const auto& a : refused)
        bad |= check(rn_jpeg::encode_info(a[0], a[1], a[2], &info) == RN_E_INVALID, "encode_info refuses", a[0], a[1]);
    std::printf("%ld files encoded into exact-size buffers and decoded back%s\n", files, bad ? ", WITH FAILURES" : ", all equal");
    return bad;
}
