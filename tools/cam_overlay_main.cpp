// Host run of the heat map's per-pixel arithmetic (roomnet_amd/csrc/rn_cam_math.h): a stand-alone program, no GPU, no HIP.
//
//   c++ -std=c++17 -O2 -ffp-contract=off -Iroomnet_amd/csrc tools/cam_overlay_main.cpp -o build/cam_overlay
//   build/cam_overlay IN OUT
//
// The device functions are compiled for the host as they stand (-ffp-contract=off for a compiler that does not know the header's
// pragma) and walked over an image the way the two kernels of rn_cam_overlay.hip walk it: the maximum of
// the upsampled window first, then colour and blend per pixel.  IN: int32 height, width, cam_h, cam_w, float64 weight, the BGR
// bytes, the float32 map.  OUT: the BGR bytes, to be compared with cam.overlay_image (tests/test_cam_overlay_host.py does, when a
// C++ compiler is there).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define __device__
#define __constant__ const
#define __forceinline__ inline
#define __restrict__
using std::floor;
using std::fmax;
using std::fmin;
using std::rint;
#include "rn_cam_math.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    int32_t hdr[4];
    double weight;
    if (!f || std::fread(hdr, 4, 4, f) != 4 || std::fread(&weight, 8, 1, f) != 1) return 2;
    const int h = hdr[0], w = hdr[1], mh = hdr[2], mw = hdr[3];
    std::vector<uint8_t> im(static_cast<size_t>(h) * w * 3);
    std::vector<float> map(static_cast<size_t>(mh) * mw);
    if (std::fread(im.data(), 1, im.size(), f) != im.size() || std::fread(map.data(), 4, map.size(), f) != map.size()) return 2;
    std::fclose(f);
    // the window of rn_center_crop_window
    const int side = h < w ? h : w, x0 = w > h ? (w - h) / 2 : 0, y0 = h > w ? (h - w + 1) / 2 : 0;
    const double sy = mh / static_cast<double>(side), sx = mw / static_cast<double>(side);
    double mx = 0.0;
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) mx = fmax(mx, rn_cam_up(map.data(), mw, rn_cam_axis_of(y, mh, sy), rn_cam_axis_of(x, mw, sx)));
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) {
            double heat[3];
            rn_cam_heat(rn_cam_up(map.data(), mw, rn_cam_axis_of(y, mh, sy), rn_cam_axis_of(x, mw, sx)), mx, heat);
            uint8_t* p = im.data() + (static_cast<size_t>(y0 + y) * w + x0 + x) * 3;
            for (int c = 0; c < 3; ++c) p[c] = static_cast<uint8_t>(rn_cam_blend(p[c], heat[c], weight, 1.0 - weight));
        }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(im.data(), 1, im.size(), f) != im.size()) return 2;
    std::fclose(f);
    return 0;
}
