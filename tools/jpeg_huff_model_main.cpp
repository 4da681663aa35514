// Host-sanitizer run of the parallel Huffman decode's host model (roomnet_amd/csrc/rn_jpeg_huff.h through rn_jpeg_huff_model.h):
// a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iroomnet_amd/csrc \
//       tools/jpeg_huff_model_main.cpp -o build/jpeg_huff_model && build/jpeg_huff_model FILE.jpg ...
//
// Every FILE (a valid baseline JPEG; tools/README.md shows how to write a few with Pillow) is walked as tools/jpeg_corrupt_main.cpp
// walks it -- truncated at 40 evenly spaced lengths, and with single bytes overwritten at 200 seeded positions with 8 values each --
// through rn_jpeg::parse, rn_jpeg::entropy_decode and rn_jpeg_huff::model at three subsequence lengths.  The input bytes and the
// coefficient buffers are heap blocks of EXACTLY the announced sizes, so AddressSanitizer sees any read or write past them.  Checked
// on every input: the model's status is 0 exactly when the sequential pass returns RN_OK -- RN_JPEG_ST_NOT_SYNCED and
// RN_JPEG_ST_TOO_LARGE excepted, which send a file to the sequential pass -- and then the coefficients are equal.
// Without arguments a built-in one-block file is used.  Prints one summary line per file, with the synchronisation rounds of the
// intact file at RN_JPEG_SUBSEQ_BYTES; exit status 0 unless a check failed (sanitizer findings abort the run themselves).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rn_jpeg_huff_model.h"

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

const int kSubseq[3] = {5, 32, RN_JPEG_SUBSEQ_BYTES};

struct Counts {
    long calls = 0, ok = 0, refused = 0, unsupported = 0, not_synced = 0, disagree = 0;
    rn_jpeg_huff::ModelRounds rounds;
};

// one input through the sequential pass and the model, on exact-size heap copies
int run_one(const unsigned char* bytes, size_t len, Counts& c, bool intact) {
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
        if (count <= (size_t(1) << 24)) {
            const rn_jpeg_info info = p.info;
            int16_t* want = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t) + 1));
            int16_t* got = static_cast<int16_t*>(std::malloc(count * sizeof(int16_t) + 1));
            const char* why = "";
            const int rc2 = rn_jpeg::entropy_decode(data, len, &info, want, count, &why);
            ++c.calls;
            if (rc2 > 0) bad = 1;
            if (rc2 == RN_OK)
                ++c.ok;
            else
                ++c.refused;
            for (const int sb : kSubseq) {
                int32_t status = -1;
                rn_jpeg_huff::ModelRounds rounds;
                const char* why3 = "";
                const int rc3 = rn_jpeg_huff::model(data, len, &info, got, count, sb, &status, &rounds, &why3);
                ++c.calls;
                if (rc3 != RN_OK || status < 0) bad = 1;
                if (status == RN_JPEG_ST_NOT_SYNCED || status == RN_JPEG_ST_TOO_LARGE) {
                    ++c.not_synced;
                    if (intact) bad = 1;
                } else if ((status == RN_JPEG_ST_OK) != (rc2 == RN_OK) ||
                           (status == RN_JPEG_ST_OK && std::memcmp(want, got, count * sizeof(int16_t)) != 0)) {
                    ++c.disagree;
                    bad = 1;
                    std::printf("  disagreement at %d-byte subsequences: status %d, sequential pass %d (%s), %zu bytes\n", sb, status, rc2,
                                rc2 == RN_OK ? "ok" : why, len);
                }
                if (intact && sb == RN_JPEG_SUBSEQ_BYTES) c.rounds = rounds;
            }
            std::free(want);
            std::free(got);
        }
    } else if (rc != RN_OK) {
        ++c.refused;
    }
    std::free(data);
    return bad;
}

int run_file(const char* name, const std::vector<unsigned char>& file) {
    Counts c;
    int bad = run_one(file.data(), file.size(), c, true);
    if (c.ok != 1) {
        std::printf("%s: the intact file did not decode\n", name);
        return 1;
    }
    for (int i = 0; i < 40; ++i) bad |= run_one(file.data(), file.size() * i / 40, c, false);
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
            bad |= run_one(hit.data(), hit.size(), c, false);
        }
        hit[pos] = file[pos];
    }
    std::printf("%s: %zu bytes, %ld calls, %ld decoded, %ld refused, %ld left to the general decoder, %ld sent back to the sequential pass, "
                "%ld disagreements; rounds of the intact file: %d inside groups, %d across%s\n",
                name, file.size(), c.calls, c.ok, c.refused, c.unsupported, c.not_synced, c.disagree, c.rounds.inside, c.rounds.across,
                bad ? ", FAILED" : "");
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
