// wz_ignore_cells (watsor_amd/csrc/wz_ignore.cpp) under the host sanitizers: a stand-alone program, no GPU, no HIP.
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/ignore_cells_check.cpp -o ignore_cells_check
//   ./ignore_cells_check
// The function walks byte planes with ragged edges -- partial last cells, rectangles at odd origins.  Every plane and every output here is
// a heap block of exactly its size, so that a read or write one byte outside it lands in a red zone; every result is compared with a
// per-cell restatement of the rule.  The shapes are those of tests/test_ignore_oracle.py.  Prints one line per case, exits 1 on a mismatch.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "../watsor_amd/csrc/wz_ignore.cpp"

static int failures = 0;

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

// a cell is ignored iff at least one pixel of it is: restated per cell
static void restate(const uint8_t* plane, int W, const wz_tile_t& r, uint8_t* cells) {
    const int cols = (r.w + 15) / 16, crows = (r.h + 15) / 16;
    for (int cy = 0; cy < crows; ++cy)
        for (int cx = 0; cx < cols; ++cx) {
            uint8_t any = 0;
            for (int y = 16 * cy; y < 16 * cy + 16 && y < r.h; ++y)
                for (int x = 16 * cx; x < 16 * cx + 16 && x < r.w; ++x)
                    if (plane[(size_t)(r.y0 + y) * W + r.x0 + x]) any = 1;
            cells[cy * cols + cx] = any;
        }
}

static void run(const char* name, int W, int H, const wz_tile_t* rect, unsigned one_in) {
    const wz_tile_t r = rect ? *rect : wz_tile_t{0, 0, W, H};
    const size_t n = (size_t)W * H, nc = (size_t)((r.w + 15) / 16) * ((r.h + 15) / 16);
    std::unique_ptr<uint8_t[]> plane(new uint8_t[n]), got(new uint8_t[nc]), want(new uint8_t[nc]);
    for (size_t i = 0; i < n; ++i) plane[i] = one_in && rnd() % one_in == 0 ? (uint8_t)(1 + rnd() % 255) : 0;
    memset(got.get(), 0xA5, nc);
    const int rc = wz_ignore_cells(plane.get(), W, H, rect, got.get());
    restate(plane.get(), W, r, want.get());
    size_t set = 0;
    for (size_t i = 0; i < nc; ++i) set += want[i];
    const bool ok = rc == WZ_OK && memcmp(got.get(), want.get(), nc) == 0;
    printf("%-34s %4dx%-4d rect (%d, %d, %d x %d)  %zu of %zu cells ignored  %s\n", name, W, H, r.x0, r.y0, r.w, r.h, set, nc, ok ? "ok" : "MISMATCH");
    if (!ok) ++failures;
}

static void refused(const char* name, int W, int H, const wz_tile_t& rect) {
    std::unique_ptr<uint8_t[]> plane(new uint8_t[(size_t)W * H]()), out(new uint8_t[1]);
    out[0] = 0xA5;
    const int rc = wz_ignore_cells(plane.get(), W, H, &rect, out.get());
    const bool ok = rc == WZ_EINVAL && out[0] == 0xA5;
    printf("%-34s %4dx%-4d rect (%d, %d, %d x %d)  %s\n", name, W, H, rect.x0, rect.y0, rect.w, rect.h, ok ? "refused, nothing written" : "NOT REFUSED");
    if (!ok) ++failures;
}

int main() {
    const unsigned densities[] = {0u, 2000u, 100u, 1u};   // none, sparse, dense, every pixel
    for (unsigned d : densities) {
        run("one cell", 16, 16, nullptr, d);
        run("63 x 5 cells, 11-pixel last ones", 1003, 75, nullptr, d);
        run("65 x 9 cells", 1040, 144, nullptr, d);
        const wz_tile_t odd = {7, 5, 100, 50};
        run("rectangle at an odd origin", 128, 64, &odd, d);
        const wz_tile_t corner = {121, 59, 7, 5};
        run("rectangle in the last corner", 128, 64, &corner, d);
        const wz_tile_t pixel = {127, 63, 1, 1};
        run("the frame's last pixel", 128, 64, &pixel, d);
        run("one pixel", 1, 1, nullptr, d);
        run("one row", 1003, 1, nullptr, d);
        run("one column", 1, 75, nullptr, d);
    }
    refused("empty", 128, 64, {0, 0, 0, 16});
    refused("negative origin", 128, 64, {-1, 0, 16, 16});
    refused("past the right edge", 128, 64, {120, 0, 9, 16});
    refused("past the bottom edge", 128, 64, {0, 60, 16, 5});
    refused("x0 + w overflows an int", 128, 64, {2147483647, 0, 2, 1});
    if (wz_ignore_cells(nullptr, 16, 16, nullptr, nullptr) != WZ_EINVAL) ++failures;
    printf("%s\n", failures ? "FAILED" : "all cases ok");
    return failures ? 1 : 0;
}
