// Host-sanitizer run of the JPEG entropy decoder (roomnet_amd/csrc/rn_jpeg_host.h): a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/jpeg_corrupt_main.cpp -o build/jpeg_corrupt && build/jpeg_corrupt FILE.jpg ...
//
// Every FILE (a valid baseline JPEG; tools/README.md shows how to write a few with Pillow) is walked as the robustness test of
// tests/test_jpegdec_host.py walks its file -- truncated at 40 evenly spaced lengths, and with single bytes overwritten at 200
// seeded positions, here with 8 values each -- through rn_jpeg::parse and rn_jpeg::entropy_decode, by the plain walk and by the
// oriented one (rn_jpeg_probe_oriented's).  Then the file gets an APP1 Exif segment with orientation 6
// spliced in behind SOI (both byte orders) and is walked again: intact, truncated at EVERY length up to the end of that segment
// and a little past it, and with every byte of the segment overwritten with 6 values.  The input bytes and the
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
    long calls = 0, ok = 0, refused = 0, unsupported = 0, turned = 0;
};

// one input through both entry points by one of the two walks, on exact-size heap copies
int run_walk(const unsigned char* bytes, size_t len, bool oriented, Counts& c) {
    unsigned char* data = static_cast<unsigned char*>(std::malloc(len ? len : 1));
    if (len) std::memcpy(data, bytes, len);
    static rn_jpeg::Parsed p;
    int bad = 0;
    const int rc = rn_jpeg::parse(data, len, p, oriented);
    ++c.calls;
    if (rc > 0) bad = 1;
    if (rc == RN_OK && (p.info.supported < 0 || p.info.supported > (oriented ? 8 : 1))) bad = 1;
    if (rc == RN_OK && p.info.supported > 1) ++c.turned;
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

int run_one(const unsigned char* bytes, size_t len, Counts& c) { return run_walk(bytes, len, false, c) | run_walk(bytes, len, true, c); }

// APP1 "Exif\0\0" whose IFD0 holds only the orientation tag (tests/jpeg_cases.py: exif_app1)
std::vector<unsigned char> exif_app1(int orientation, bool le) {
    std::vector<unsigned char> s = {0xff, 0xe1, 0x00, 0x22, 'E', 'x', 'i', 'f', 0, 0};
    auto u16 = [&](unsigned v) {
        s.push_back(static_cast<unsigned char>(le ? v & 255 : v >> 8));
        s.push_back(static_cast<unsigned char>(le ? v >> 8 : v & 255));
    };
    auto u32 = [&](unsigned v) {
        u16(le ? v & 0xffff : v >> 16);
        u16(le ? v >> 16 : v & 0xffff);
    };
    s.push_back(le ? 'I' : 'M');
    s.push_back(le ? 'I' : 'M');
    u16(42);
    u32(8);
    u16(1);
    u16(0x0112);
    u16(3);
    u32(1);
    u16(static_cast<unsigned>(orientation));
    u16(0);
    u32(0);
    return s;      // 36 bytes: marker, length 34, 32 bytes of payload
}

// the spliced file: intact (must decode as orientation 6), every truncation through the segment, every byte of it overwritten
int run_spliced(const char* name, const std::vector<unsigned char>& file, bool le, Counts& c) {
    const std::vector<unsigned char> app1 = exif_app1(6, le);
    std::vector<unsigned char> sp(file.begin(), file.begin() + 2);
    sp.insert(sp.end(), app1.begin(), app1.end());
    sp.insert(sp.end(), file.begin() + 2, file.end());
    Counts intact;
    int bad = run_walk(sp.data(), sp.size(), true, intact);
    if (intact.ok != 1 || intact.turned != 1) {
        std::printf("%s: the spliced file did not decode as a turned one\n", name);
        return 1;
    }
    Counts plain;
    bad |= run_walk(sp.data(), sp.size(), false, plain);
    if (plain.unsupported != 1) {
        std::printf("%s: the plain walk did not leave the spliced file to the general decoder\n", name);
        return 1;
    }
    const size_t end = 2 + app1.size();
    for (size_t n = 0; n <= end + 16 && n <= sp.size(); ++n) bad |= run_one(sp.data(), n, c);
    std::vector<unsigned char> hit(sp);
    const unsigned char values[6] = {0x00, 0xff, 0x01, 0x06, 0x80, 0x7f};
    for (size_t pos = 2; pos < end; ++pos) {
        for (const unsigned char v : values) {
            hit[pos] = v;
            bad |= run_one(hit.data(), hit.size(), c);
        }
        hit[pos] = sp[pos];
    }
    return bad;
}

int run_file(const char* name, const std::vector<unsigned char>& file) {
    Counts c;
    int bad = run_one(file.data(), file.size(), c);
    if (c.ok != 2) {          // (once by each walk)
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
    for (const bool le : {true, false}) {
        bad |= run_spliced(name, file, le, c);
    }
    std::printf("%s: %zu bytes, %ld calls, %ld decoded, %ld probed as turned, %ld refused, %ld left to the general decoder%s\n", name,
                file.size(), c.calls, c.ok, c.turned, c.refused, c.unsupported, bad ? ", POSITIVE RETURN CODE OR A FIELD OUT OF RANGE" : "");
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
