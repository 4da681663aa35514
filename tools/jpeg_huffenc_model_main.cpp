// Host-sanitizer run of the parallel Huffman ENCODE's host model (roomnet_amd/csrc/rn_jpeg_huffenc.h): a stand-alone program,
// no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/jpeg_huffenc_model_main.cpp -o build/jpeg_huffenc_model && build/jpeg_huffenc_model
//
// For several sizes (one MCU, odd sizes, more than one scan tile, more than one stuffing chunk) seeded random in-range
// coefficient arrays -- sparse, dense, long zero runs, all AC 1023 (FF bytes in pairs) -- and hand-built blocks go through the
// model (the phases of rn_jpeg_huffenc.hip, work item after work item through the same piece()): once with a cap of 0 to learn
// the length, then into a heap block of EXACTLY that many bytes, so AddressSanitizer sees any write past it, and the file is
// compared with rn_jpeg::entropy_encode's.  Then the refusals: a cap one byte short (status CAP, the length reported), values
// beyond the Huffman categories (status CATEGORY exactly where entropy_encode returns RN_E_INVALID), an info with more blocks
// than 32-bit bit offsets address (status TOO_LARGE with a one-block coefficient array: it is not read), infos the encoder does
// not write (RN_E_INVALID).  Prints one summary line; exit status 0 unless something differed (sanitizer findings abort the run).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rn_jpeg_huffenc.h"

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
            if (mode == 3) {
                blk[k] = 1023;
                continue;
            }
            const bool zero = mode == 0 ? next() % 5 != 0 : (mode == 1 ? false : k != 63 && k != 17);
            blk[k] = zero ? 0 : static_cast<int16_t>(in_range(1023));
        }
    }
}

int check(bool ok, const char* what, int w, int h) {
    if (!ok) std::printf("FAILED: %s (%dx%d)\n", what, w, h);
    return ok ? 0 : 1;
}

// the model into an exact-size block against entropy_encode; a cap one byte short
int compare(const rn_jpeg_info& info, const std::vector<int16_t>& c, long& files) {
    const int w = info.width, h = info.height;
    const size_t count = c.size();
    const char* why = "";
    int16_t* coeffs = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t)));      // (a read past the coefficients is seen as well)
    std::memcpy(coeffs, c.data(), count * sizeof(int16_t));
    std::vector<uint8_t> ref(rn_jpeg::encoded_bound(info));
    size_t ref_len = 0, len = 0, len2 = 0;
    int32_t status = -1;
    int bad = check(rn_jpeg::entropy_encode(&info, coeffs, ref.data(), ref.size(), &ref_len, &why) == RN_OK, "the reference encodes", w, h);
    bad |= check(rn_jpeg_huffenc::model(&info, coeffs, nullptr, 0, &len, &status, &why) == RN_OK && status == RN_JPEG_ENC_ST_CAP && len == ref_len,
                 "cap 0 is status CAP with the length", w, h);
    uint8_t* out = static_cast<uint8_t*>(std::malloc(len));
    bad |= check(rn_jpeg_huffenc::model(&info, coeffs, out, len, &len2, &status, &why) == RN_OK && status == RN_JPEG_ENC_ST_OK && len2 == len &&
                     std::memcmp(out, ref.data(), len) == 0,
                 "the model's file equals entropy_encode's", w, h);
    uint8_t* shorter = static_cast<uint8_t*>(std::malloc(len - 1));
    bad |= check(rn_jpeg_huffenc::model(&info, coeffs, shorter, len - 1, &len2, &status, &why) == RN_OK && status == RN_JPEG_ENC_ST_CAP && len2 == len,
                 "cap len - 1 is status CAP", w, h);
    std::free(shorter);
    std::free(out);
    std::free(coeffs);
    ++files;
    return bad;
}

int run_size(int w, int h, int quality, long& files) {
    rn_jpeg_info info;
    int bad = check(rn_jpeg::encode_info(w, h, quality, &info) == RN_OK, "encode_info", w, h);
    if (bad) return bad;
    const size_t count = rn_jpeg::coeff_count(info);
    std::vector<int16_t> c(count);
    for (int mode = 0; mode < 4; ++mode) {
        fill(c, mode);
        bad |= compare(info, c, files);
    }
    // hand-built blocks: a lone value at zigzag 63 (three ZRL, no EOB), 17 (one ZRL), 16 (run 15), the top categories
    for (const int zz : {63, 17, 16}) {
        std::fill(c.begin(), c.end(), static_cast<int16_t>(0));
        for (size_t b = 0; b < count / 64; b += 2) c[b * 64 + rn_jpeg::kNatural[zz]] = static_cast<int16_t>(b % 3 ? -3 : 5);
        bad |= compare(info, c, files);
    }
    std::fill(c.begin(), c.end(), static_cast<int16_t>(0));
    for (size_t b = 0; b < count / 64; ++b) {
        c[b * 64] = static_cast<int16_t>(b % 2 ? -1024 : 1023);          // differences of +-2047 inside a component
        c[b * 64 + 1 + b % 63] = static_cast<int16_t>(b % 2 ? -1023 : 1023);
    }
    bad |= compare(info, c, files);
    // what entropy_encode refuses in the coefficients is status CATEGORY, and nothing else is
    const char* why = "";
    std::vector<uint8_t> buf(rn_jpeg::encoded_bound(info));
    auto agree = [&](const char* what, bool refused) {
        size_t len = 0;
        int32_t status = -1;
        const int ref = rn_jpeg::entropy_encode(&info, c.data(), buf.data(), buf.size(), &len, &why);
        const int rc = rn_jpeg_huffenc::model(&info, c.data(), buf.data(), buf.size(), &len, &status, &why);
        return check(ref == (refused ? RN_E_INVALID : RN_OK) && rc == RN_OK && status == (refused ? RN_JPEG_ENC_ST_CATEGORY : RN_JPEG_ENC_ST_OK), what, w, h);
    };
    std::fill(c.begin(), c.end(), static_cast<int16_t>(0));
    c[9] = 1023;
    bad |= agree("AC 1023 is accepted", false);
    c[9] = 1024;
    bad |= agree("AC 1024 is status CATEGORY", true);
    c[9] = -32768;
    bad |= agree("AC -32768 is status CATEGORY", true);
    c[9] = 0;
    c[0] = 2047;
    bad |= agree("DC difference 2047 is accepted", false);
    c[0] = 2048;
    bad |= agree("DC difference 2048 is status CATEGORY", true);
    c[0] = 32767;
    c[64] = -32768;
    bad |= agree("DC difference 65535 is status CATEGORY", true);
    c[0] = c[64] = 0;
    // infos the encoder does not write
    size_t len = 0;
    int32_t status = -1;
    rn_jpeg_info other = info;
    other.ncomp = 1;
    other.hsamp = other.vsamp = 1;
    bad |= check(rn_jpeg_huffenc::model(&other, c.data(), buf.data(), buf.size(), &len, &status, &why) == RN_E_INVALID, "grey is RN_E_INVALID", w, h);
    other = info;
    other.blocks_h[2] += 1;
    bad |= check(rn_jpeg_huffenc::model(&other, c.data(), buf.data(), buf.size(), &len, &status, &why) == RN_E_INVALID, "an inconsistent grid is RN_E_INVALID", w, h);
    bad |= check(rn_jpeg_huffenc::model(&info, nullptr, buf.data(), buf.size(), &len, &status, &why) == RN_E_INVALID, "null coefficients are RN_E_INVALID", w, h);
    size_t head = 0;
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(rn_jpeg::kEncHeaderBytes));
    bad |= check(rn_jpeg_huffenc::encode_headers(&info, exact, rn_jpeg::kEncHeaderBytes, &head, &why) == RN_OK && head == rn_jpeg::kEncHeaderBytes,
                 "the headers take kEncHeaderBytes", w, h);
    bad |= check(rn_jpeg_huffenc::encode_headers(&info, exact, rn_jpeg::kEncHeaderBytes - 1, &head, &why) == RN_E_RANGE, "headers into a short buffer", w, h);
    std::free(exact);
    return bad;
}

}  // namespace

int main() {
    // 16x16: one MCU; 320x240: 1800 blocks, 8 scan tiles; 640x480 dense: several hundred stuffing chunks
    const int sizes[][2] = {{1, 1}, {8, 8}, {16, 16}, {17, 33}, {53, 37}, {2, 31}, {49, 50}, {96, 72}, {200, 120}, {320, 240}, {640, 480}};
    int bad = 0;
    long files = 0;
    for (const auto& s : sizes) bad |= run_size(s[0], s[1], 100, files);
    bad |= run_size(53, 37, 30, files);
    // too large: decided from the info alone -- the coefficient block holds ONE block
    rn_jpeg_info info;
    bad |= check(rn_jpeg::encode_info(16384, 16384, 95, &info) == RN_OK, "encode_info", 16384, 16384);
    int16_t* one = static_cast<int16_t*>(std::calloc(64, sizeof(int16_t)));
    size_t len = 1;
    int32_t status = -1;
    const char* why = "";
    bad |= check(rn_jpeg_huffenc::model(&info, one, nullptr, 0, &len, &status, &why) == RN_OK && status == RN_JPEG_ENC_ST_TOO_LARGE && len == 0,
                 "more than RN_JPEG_HUFFENC_MAX_BLOCKS blocks is status TOO_LARGE", 16384, 16384);
    std::free(one);
    std::printf("%ld coefficient sets through the model into exact-size buffers%s\n", files, bad ? ", WITH FAILURES" : ", all equal to entropy_encode");
    return bad;
}
