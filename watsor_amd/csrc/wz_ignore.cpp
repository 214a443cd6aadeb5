// Ignore masks, host side (include/watsor_hip.h: wz_ignore_cells): the one place the cell rule is written.
//
// A camera's ignore plane is height x width bytes, nonzero = ignore.  The kernels never see it: they see one bit per cell of
// WZ_GATE_CELL x WZ_GATE_CELL pixels of the grid they compare -- the frame's grid, anchored at the frame's origin, for a motion camera; a
// tile's own grid, anchored at the tile's origin, for a gated one -- and a cell is ignored iff AT LEAST ONE pixel of it is ignored in the
// plane (the last column and row of cells are partial: only their pixels inside the rectangle count).  wz_tiles.hip packs what this
// function returns into the words the kernels read.  No HIP here: the function needs no engine and no device.
#include <stdint.h>

#include "../../include/watsor_hip.h"

extern "C" int wz_ignore_cells(const uint8_t* ignore, int width, int height, const wz_tile_t* rect, uint8_t* cells) {
    if (!ignore || !cells || width < 1 || height < 1) return WZ_EINVAL;
    const wz_tile_t whole = {0, 0, width, height};
    const wz_tile_t r = rect ? *rect : whole;
    if (r.w < 1 || r.h < 1 || r.x0 < 0 || r.y0 < 0 || (int64_t)r.x0 + r.w > width || (int64_t)r.y0 + r.h > height) return WZ_EINVAL;
    const int cols = (r.w + WZ_GATE_CELL - 1) / WZ_GATE_CELL, crows = (r.h + WZ_GATE_CELL - 1) / WZ_GATE_CELL;
    for (int cy = 0; cy < crows; ++cy) {
        uint8_t* out = cells + (size_t)cy * cols;
        for (int cx = 0; cx < cols; ++cx) out[cx] = 0;
        const int y1 = cy * WZ_GATE_CELL + WZ_GATE_CELL < r.h ? cy * WZ_GATE_CELL + WZ_GATE_CELL : r.h;
        for (int y = cy * WZ_GATE_CELL; y < y1; ++y) {
            const uint8_t* row = ignore + (size_t)(r.y0 + y) * (size_t)width + r.x0;
            for (int x = 0; x < r.w; ++x)
                if (row[x]) out[x / WZ_GATE_CELL] = 1;
        }
    }
    return WZ_OK;
}
