// image_fill.h -- what the batched input fill (image_fill.hip) shares with the device JPEG pixel stage
// (jpeg_pixels.hip), which produces the uint8 pixels on the device and then runs the same fill kernel on them: the
// per-image record, its geometry and tap tables (which augment.hip's letterbox kernel reads as well), and the launch of
// fill_images_kernel. The pinned staging block itself is the slot STAGE_IMAGES of the library's table (common.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace bcnn_hip {

// Per-image record at the head of the staging block. Offsets count from the block's first byte.
struct ImageDesc {
    uint32_t data_off;           // packed pixels: h rows of w * c bytes (the caller's row padding is dropped)
    uint32_t tapx_off, tapy_off; // int2 (index, frac) per column of the resized image / per row
    int w, h;                    // source extent
    int new_w, new_h;            // extent of the resized image inside the W x H plane
    int x_off, y_off;            // where it is pasted; everything outside is the canvas value 128
};

// Extent of image iw x ih inside the W x H plane (stretch or letterbox); false when an extent comes out 0.
bool fitted_extent(int fit, int W, int H, int iw, int ih, int* new_w, int* new_h);
// d.w, d.h, d.new_w and d.new_h are set: writes the tap tables of the resize (new_w columns, then new_h rows) at
// stage + tap_at and d.tapx_off / d.tapy_off; returns the bytes written.
size_t stage_taps(uint8_t* stage, size_t tap_at, ImageDesc& d);
// Fills d (all but data_off) and the tap tables of an iw x ih image at stage + tap_at; returns the bytes of taps written.
size_t stage_geometry(uint8_t* stage, size_t tap_at, ImageDesc& d, int fit, int W, int H, int iw, int ih);
// Grid of the fill kernel for num_images planes of W x H; false when it does not fit 31 bits.
bool fill_grid(int W, int H, int num_images, int* runs_per_row, int* blocks_per_image, long long* blocks);
// Queues fill_images_kernel<c> on st: descriptors, taps and pixels are in the device block stage_d.
void launch_fill_images(const uint8_t* stage_d, float* dst_d, int c, int H, int W, int num_images, float norm_coeff,
                        int swap_to_bgr, float mean_r, float mean_g, float mean_b, hipStream_t st);

}  // namespace bcnn_hip
