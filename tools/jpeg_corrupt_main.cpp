// Host-sanitizer run of the JPEG entropy decoder (roomnet_amd/csrc/rn_jpeg_host.h): a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/jpeg_corrupt_main.cpp -o build/jpeg_corrupt && build/jpeg_corrupt FILE.jpg ...
//
// Every FILE (a valid baseline JPEG; tools/README.md shows how to write a few with Pillow) is walked as the robustness test of
// tests/test_jpegdec_host.py walks its file -- truncated at 40 evenly spaced lengths, and with single bytes overwritten at 200
// seeded positions, here with 8 values each -- through rn_jpeg::parse and rn_jpeg::entropy_decode.  The input bytes and the
// coefficient buffer are heap blocks of EXACTLY the announced sizes, so AddressSanitizer sees any read or write past them.
// Without arguments a built-in one-block file is used.  Prints one summary line per file; exit status 0 unless a call returned
// a positive code or an intact file failed to decode (sanitizer findings abort the run themselves).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rn_jpeg_host.h"

namespace {

// the one-block grey file of tests/jpeg_cases.py: hand_built_grey_8x8(1, 1096, -1096)
const unsigned char kBuiltin[] = {
    0xff, 0xd8, 0xff, 0xdb, 0x00, 0x43, 0x00, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01,
    0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01,
    0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01,
    0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0x01, 0xff, 0xc0, 0x00, 0x0b, 0x08, 0x00, 0x08, 0x00, 0x08,
    0x01, 0x01, 0x11, 0x00, 0xff, 0xc4, 0x00, 0x16, 0x00, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00,
    0x00, 0x00, 0x00, 0x00, 0x00, 0x0b, 0x00, 0x0a, 0xff, 0xc4, 0x00, 0x16, 0x10, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00,
    0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x0b, 0x0a, 0xff, 0xda, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00,
    0x3f, 0x00, 0x22, 0x42, 0xed, 0xcf, 0xff, 0xd9};

struct Counts {
    long calls = 0, ok = 0, refused = 0, unsupported = 0;
};

// one input through both entry points, on exact-size heap copies
int run_one(const unsigned char* bytes, size_t len, Counts& c) {
    unsigned char* data = static_cast<unsigned char*>(std::malloc(len ? len : 1));
    if (len) std::memcpy(data, bytes, len);
    static rn_jpeg::Parsed p;
    int bad = 0;
    const int rc = rn_jpeg::parse(data, len, p);
    ++c.calls;
    if (rc > 0) bad = 1;
    if (rc == RN_OK && !p.info.supported) ++c.unsupported;
    if (rc == RN_OK && p.info.supported) {
        const size_t count = rn_jpeg::coeff_count(p.info);
        if (count <= (size_t(1) << 26)) {
            const rn_jpeg_info info = p.info;
            int16_t* coeffs = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t) + 1));
            const char* why = "";
            const int rc2 = rn_jpeg::entropy_decode(data, len, &info, coeffs, count, &why);
            ++c.calls;
            if (rc2 > 0) bad = 1;
            if (rc2 == RN_OK)
                ++c.ok;
            else
                ++c.refused;
            std::free(coeffs);
        }
    } else if (rc != RN_OK) {
        ++c.refused;
    }
    std::free(data);
    return bad;
}

int run_file(const char* name, const std::vector<unsigned char>& file) {
    Counts c;
    int bad = run_one(file.data(), file.size(), c);
    if (c.ok != 1) {
        std::printf("%s: the intact file did not decode\n", name);
        return 1;
    }
    for (int i = 0; i < 40; ++i) bad |= run_one(file.data(), file.size() * i / 40, c);
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    std::vector<unsigned char> hit(file);
    for (int i = 0; i < 200; ++i) {
        const size_t pos = next() % file.size();
        for (int k = 0; k < 8; ++k) {
            hit[pos] = static_cast<unsigned char>(k == 0 ? 0xff : (k == 1 ? 0x00 : next() & 255));
            bad |= run_one(hit.data(), hit.size(), c);
        }
        hit[pos] = file[pos];
    }
    std::printf("%s: %zu bytes, %ld calls, %ld decoded, %ld refused, %ld left to the general decoder%s\n", name, file.size(), c.calls,
                c.ok, c.refused, c.unsupported, bad ? ", POSITIVE RETURN CODE" : "");
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    int bad = 0;
    if (argc < 2) bad |= run_file("built-in", std::vector<unsigned char>(kBuiltin, kBuiltin + sizeof(kBuiltin)));
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::printf("%s: cannot open\n", argv[a]);
            return 2;
        }
        std::vector<unsigned char> file;
        unsigned char buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + n);
        std::fclose(f);
        if (file.empty()) {
            std::printf("%s: empty\n", argv[a]);
            return 2;
        }
        bad |= run_file(argv[a], file);
    }
    return bad;
}
