// The per-scene uniform grid of csrc/knn_grid.hip, for the translation units that walk it (knn_grid.hip, point_group.hip): the scene
// record, the workspace layout and the two index helpers.  The kernels that BUILD the grid live in knn_grid.hip alone.
#pragma once
#include "pdfops_common.h"

namespace kg {

constexpr int CAP_CELLS = 1 << 20;  // cells per scene
// The radius queries accept d2 < r^2 OR d2 <= 1e-5: whatever the radius, a query reaches sqrt(1e-5) = 3.16228 mm.  Their 27 cells cover the
// accepted set only if the cell is at least that wide, so the cell bound is max(radius, this) -- the same cell as before for every radius
// from 3.1623 mm up; below it (the adaptive radius of a flat or thin scene: pad / divisor) the bound is what keeps the table exact.
constexpr float RQ_MIN_REACH = 3.1623e-3f;
constexpr int PB = 256;

struct SceneGrid {      // 16 floats / ints per scene in the workspace
    float minx, miny, minz, inv_h;
    float h;
    int nx, ny, nz;
    int start, n;       // source point range
    int cell_base;      // offset of this scene's cells in the cell arrays
    int pad[5];
};

struct Layout {
    size_t grid, cell_start, cursor, cell_of, sorted, redo, total;
};
__host__ __device__ inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }
__host__ __device__ inline Layout make_layout(int b, int n, int m) {
    Layout L;
    size_t o = 0;
    L.grid = o;       o = al(o + (size_t)b * sizeof(SceneGrid));
    L.cell_start = o; o = al(o + ((size_t)b * CAP_CELLS + 1) * 4);
    L.cursor = o;     o = al(o + (size_t)b * CAP_CELLS * 4);
    L.cell_of = o;    o = al(o + (size_t)n * 4);
    L.sorted = o;     o = al(o + (size_t)n * 16);
    L.redo = o;       o = al(o + ((size_t)m + 4) * 4);
    L.total = o;
    return L;
}

__device__ __forceinline__ int cell_coord(float v, float lo, float inv_h, int n) {
    int c = (int)floorf((v - lo) * inv_h);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

__device__ __forceinline__ int scene_of(int i, const int *__restrict__ offset, int b) {
    int s = 0;
    while (s < b - 1 && i >= offset[s]) ++s;
    return s;
}

}  // namespace kg

// The grid of `n` source points with cells at least `min_cell` wide (so that the 27 cells around a point cover its ball of that radius), in
// a workspace of make_layout(b, n, 0).total bytes: scene records, cell starts and the cell-sorted copy {x, y, z, index}.  Launches only
// (the counts are zeroed by a kernel, no memset node); 1 <= b <= 64.  Defined in knn_grid.hip.
int pdf_grid_build_min_cell(int n, const float *xyz, const int *offset, int b, float min_cell, void *workspace, long workspace_bytes,
                            void *stream);
