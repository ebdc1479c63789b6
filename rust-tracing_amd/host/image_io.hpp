// Image ingest for ImageTexture (reference: image::io::Reader::open(path).decode(), src/texture.rs:78) and
// PNG, Radiance .hdr and PFM output for render() (reference: image::codecs::png::PngEncoder, src/renderer.rs:59-72).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace rt {

// The readers refuse a file that announces more pixels than this before allocating anything for it (2^28: a 16 384 x 16 384 texture)
constexpr uint64_t MAX_IMAGE_PIXELS = 1ull << 28;

struct ImageRGB8 {
    int32_t width = 0, height = 0;
    std::shared_ptr<const std::vector<uint8_t>> pixels; // row-major RGB8, row 0 = top
};

// Accepts: "synthetic:WxH" (deterministic integer-only procedural earth-like map, used where the reference's
// assets/earth-large.jpg is not available), binary PPM (P6, maxval 255), JPEG (sequential or progressive, 8-bit) and
// PNG (every bit depth, plain or Adam7-interlaced).
// Throws std::runtime_error on failure (the reference panics: `.unwrap()`, src/texture.rs:78).
ImageRGB8 load_image_rgb8(const std::string &path);

ImageRGB8 synthetic_earth(int32_t width, int32_t height);

// RGB8 PNG, zlib-deflated, adaptive per-row filter.  Returns false on I/O failure.
bool write_png_rgb8(const std::string &path, int32_t width, int32_t height, const uint8_t *rgb);

// The film formats' files (include/rt_amd.h "film output"), each from the frame rt_film_device / rth_film writes in its format; false on
// I/O failure.
//   write_png_rgb16: native-endian uint16 samples as a PNG of colour type 2 and bit depth 16, through write_png_rgb8's filter and zlib path.
//   write_hdr_rgbe:  R, G, B, E bytes as a Radiance picture, "#?RADIANCE / FORMAT=32-bit_rle_rgbe / -Y h +X w", top row first; scanlines
//                    of 8 .. 32767 pixels in the new-style run-length code (2 2 hi lo, then the four byte planes), others as flat pixels.
//   write_pfm_rgb:   floats as a colour PFM, "PF / w h / -1.0": little-endian, the bottom row first.
bool write_png_rgb16(const std::string &path, int32_t width, int32_t height, const uint16_t *rgb);
bool write_hdr_rgbe(const std::string &path, int32_t width, int32_t height, const uint8_t *rgbe);
bool write_pfm_rgb(const std::string &path, int32_t width, int32_t height, const float *rgb);

// write_pfm_rgb's counterpart, for a reference frame a user hands in (include/rt_amd.h "frame metrics"): a colour PFM ("PF", width,
// height and scale separated by white space, exactly one white-space character behind the scale, then rows of RGB f32, the bottom row
// first; a negative scale means little-endian, a positive one big-endian; its magnitude is not applied).  `out`, if not null, receives
// 3 * w * h doubles, row 0 on top, each the file's f32 widened.  Every header number is bounded before it is multiplied: refused are a
// width or height < 1 or of more than nine digits, width x height >= 2^27, a scale that is zero, not finite or not a number to its last
// character, and a body shorter than the header announces; nothing beyond `size` is read.  Returns "" or the reason.
constexpr int64_t PFM_MAX_PIXELS = (int64_t)1 << 27;
std::string parse_pfm_rgb(const uint8_t *data, size_t size, int32_t &width, int32_t &height, std::vector<double> *out);
std::string read_pfm_rgb(const std::string &path, int32_t &width, int32_t &height, std::vector<double> *out);

} // namespace rt
