// vh_png.cpp -- 8-bit RGBA PNG writer on the system zlib (what renderToFile saves; the reference writes JPEG through
// FreeImage, DSC/DepthSensing.cpp:1150-1255).  Lossless, so a test can compare the pixels it reads back.  No HIP in here.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vh_api.h"

namespace {

void put32(std::vector<unsigned char>& out, uint32_t v)
{
    for (int s = 24; s >= 0; s -= 8) out.push_back((unsigned char)(v >> s));
}

// length, type, data, CRC over type and data (PNG specification, section 5.3)
void chunk(std::vector<unsigned char>& out, const char type[4], const unsigned char* data, size_t n)
{
    put32(out, (uint32_t)n);
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data, data + n);
    put32(out, (uint32_t)crc32(0L, out.data() + at, (uInt)(n + 4)));
}

} // namespace

extern "C" int vh_write_png_rgba8(const char* filename, uint32_t width, uint32_t height, const uint8_t* rgba, int level)
{
    if (!filename || !rgba || width == 0 || height == 0 || level < -1 || level > 9) return VH_ERR_BAD_ARGUMENT;
    // every row gets filter type 0 (none) in front of its bytes
    const size_t row = (size_t)width * 4;
    std::vector<unsigned char> raw((row + 1) * height);
    for (uint32_t y = 0; y < height; y++) {
        raw[y * (row + 1)] = 0;
        std::memcpy(&raw[y * (row + 1) + 1], rgba + y * row, row);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<unsigned char> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), level) != Z_OK) return VH_ERR_IO;

    std::vector<unsigned char> out = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n' };
    std::vector<unsigned char> ihdr;
    put32(ihdr, width);
    put32(ihdr, height);
    ihdr.insert(ihdr.end(), { 8, 6, 0, 0, 0 }); // bit depth 8, colour type 6 (RGBA), deflate, adaptive filters, no interlace
    chunk(out, "IHDR", ihdr.data(), ihdr.size());
    chunk(out, "IDAT", z.data(), zn);
    chunk(out, "IEND", nullptr, 0);

    FILE* f = std::fopen(filename, "wb");
    if (!f) return VH_ERR_IO;
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? VH_OK : VH_ERR_IO;
}
