// What a handle keeps for the JPEG decode stages, shared by the pixel stage (rn_jpeg.hip) and the Huffman stage (rn_jpeg_huff.hip):
// scratch that only grows, two sets of the batch tables behind ONE rotation (rn_batch_table.h), the events that order the copy
// stream against the scratch, one interval timer per stage.
#pragma once
#include "rn_internal.h"
#include "rn_jpeg_huff.h"

#include <vector>

struct JpegDev {
    const int16_t* coef[3];   // [blocks_h][blocks_w][64] per component
    uint8_t* plane[3];        // [blocks_h * 8][blocks_w * 8] per component
    uint8_t* bgr;             // [height][width][3]; orient 5..8: [width][height][3]
    int32_t width, height, ncomp, hsamp, vsamp;      // the STORED size
    int32_t orient;           // EXIF orientation 1..8 the store turns the pixels by
    int32_t bw[3], bh[3];
    uint16_t qt[3][64];
};

// one image of the Huffman stage's launches
struct HuffDev {
    const uint8_t* scan;                   // device, scan_len bytes
    const rn_jpeg_huff::Tables* tables;    // device
    rn_jpeg_huff::State* exit_state;       // [nsub] what the decoder of subsequence i leaves
    uint32_t* base;                        // [nsub] blocks of the scan in front of subsequence i
    int16_t* coef[3];
    uint32_t scan_len, nsub;               // nsub 0: the host decided the status, the kernels pass the image by
    int32_t nblk[3], q0[3];
    rn_jpeg_huff::Geom g;
};

struct JpegState {
    int16_t* d_coef = nullptr;
    size_t coef_cap = 0;          // int16 elements
    uint8_t* d_planes = nullptr;
    size_t planes_cap = 0;
    uint8_t* d_bgr = nullptr;     // rn_classify_jpegs: the decoded images
    size_t bgr_cap = 0;
    rn_table<JpegDev> desc[2];    // [max_batch]
    rn_rotation turn;
    std::vector<uint8_t*> bgr_ptrs;
    hipEvent_t uploaded = nullptr, done = nullptr;
    rn_timer timer;
    bool ready = false;
    // the Huffman stage (allocated by its first call)
    uint8_t* d_scan = nullptr;    // the batch's scan bytes
    size_t scan_cap = 0;
    uint8_t* d_chain = nullptr;   // per subsequence: exit state, block base
    size_t chain_cap = 0;
    rn_table<HuffDev> huff[2];                    // [max_batch]
    rn_table<rn_jpeg_huff::Tables> huff_tables[2];
    rn_table<int32_t> huff_status[2];
    rn_table<int32_t> huff_rounds[2];             // [2 * max_batch] rounds phase 2 took: inside groups (most), across groups
    int last_set = 0;                              // the set of the last Huffman call
    hipEvent_t scan_done = nullptr;
    rn_timer huff_timer;
    bool huff_ready = false;
};

// one image of the pixel stage: its coefficients in host memory (uploaded) or already in device memory
struct rn_jpeg_job {
    const rn_jpeg_info* info;
    const int16_t* coeffs;
    bool on_device;
};

// (rn_jpeg.hip)
int rn_jpeg_state(rn_handle* h, JpegState** out);
bool rn_jpeg_info_ok(const rn_jpeg_info& f);
// the size of the image the pixel stage leaves for a checked info: the stored one, swapped for orientations 5..8
inline int rn_jpeg_out_height(const rn_jpeg_info& f) { return f.supported >= 5 ? f.width : f.height; }
inline int rn_jpeg_out_width(const rn_jpeg_info& f) { return f.supported >= 5 ? f.height : f.width; }
// upload + the two pixel-stage launches, then crop + resize + forward pass, results to the host: the body of rn_classify_jpegs
int rn_jpeg_classify_jobs(rn_handle* h, JpegState* st, const rn_jpeg_job* jobs, int n, float* probs, int64_t* ids);
