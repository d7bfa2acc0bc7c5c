// jpeg_pixels.h -- what the device JPEG pixel stage (jpeg_pixels.hip) shares with the loader's device-decode path
// (augment.hip), which lays coefficient blocks out in its own staging block and runs the same two kernels on them: the
// frame check, the sizes of one frame, the plane / image tables and the launch of jpeg_idct_kernel + jpeg_colour_kernel.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/bcnn_hip.h"

namespace bcnn_hip {

// A frame the two kernels can run on without leaving its planes (ncomp == c, c 1 or 3, numbers that fit together).
bool jpeg_frame_ok(const bcnn_hip_jpeg_frame& f, int c);

// What one checked frame takes: bytes of coefficients, planes and interleaved pixels (each a multiple of 16), 8 x 8 blocks
// the IDCT kernel transforms, runs of 8 pixels the colour kernel converts.
struct JpegFrameSize { size_t coeff, planes, pixels; unsigned long long blocks, runs; };
JpegFrameSize jpeg_frame_size(const bcnn_hip_jpeg_frame& f, int c);

// The two tables, each closed by a record that holds only the total; bytes, multiples of 16.
size_t jpeg_plane_table_bytes(int num_planes);
size_t jpeg_image_table_bytes(int num_images);

// Where the next image goes while a batch is laid out: offsets in bytes from the block's first byte (multiples of 16,
// below 2^31), totals so far.
struct JpegCursor {
    size_t coeff_at, plane_at, pixel_at;
    uint32_t block_at, run_at;
    int planes, images;
};
// Appends image `cur.images` (coefficients at cur.coeff_at, planes from cur.plane_at, pixels at cur.pixel_at) to the
// tables at stage + planes_at / images_at and moves the cursor behind it. jpeg_close_tables writes the two end records.
void jpeg_append_image(uint8_t* stage, size_t planes_at, size_t images_at, const bcnn_hip_jpeg_frame& f, int c,
                       JpegCursor& cur);
void jpeg_close_tables(uint8_t* stage, size_t planes_at, size_t images_at, const JpegCursor& cur);
// Queues the two kernels on st over the tables of the device block stage_d; nothing when the cursor holds no image.
void launch_jpeg_pixels(uint8_t* stage_d, uint32_t planes_off, uint32_t images_off, const JpegCursor& cur, hipStream_t st);

}  // namespace bcnn_hip
