// The cell-pruned farthest-point sampler's launch arguments (ag_fps_grid.hip; entry point ag_fps_cloud_grid in ag_api_cells.hip).
// Internal.
#pragma once
#include "ag_common.h"

namespace ag {

constexpr int FPS_GRID_MAX_NOBJ = 1 << 16, FPS_GRID_MAX_POINTS = 1 << 20;
constexpr int FPS_GRID_CELL_POINTS = 64;         // the default policy: about this many points per cell,
constexpr int FPS_GRID_MAX_CELLS = 1 << 14;      // a power-of-two cell count per cloud, at most this
constexpr int FPS_GRID_LDS_CELLS = 2048;         // up to here the per-cell tables of the selection live in LDS

// One binning pass's scratch for B clouds of up to P points in up to CC cells each (+ 1 for the non-finite points).  All of it is
// written before it is read; `zeroed` is cleared by the launch.
struct FpsBinWs {
    int cells_cap;                                // CC
    unsigned* zeroed; size_t zeroed_words;        // per cloud [6 ordered bounds | CC + 1 counts]
    char* grid;                                   // B x fps_grid_bytes()
    int* start;                                   // (B, CC + 2)
    int* cid; int* slot;                          // (B, P)
    float* sorted;                                // (B, P, 4): x, y, z, original index; 16-byte aligned
    float* md;                                    // (B, P): running minima in cell order
    float* box;                                   // (B, CC + 1, 6): lo xyz, hi xyz, cell order
    unsigned long long* key0;                     // (B, CC + 1): initial packed max keys
    char* tab;                                    // selection tables beyond LDS: B x fps_grid_tab_bytes(CC), else unused
};
struct FpsGridArgs {
    const float* pos; const long long* pt_off; const long long* npts; int stride;
    const int* fps_start; const float* fps_radius; const int* rad_start;
    int B, max_nobj, max_pts, cells;              // cells: 0 = the default policy, else the forced power of two
    int* fps_idx; int* n_obj;
    FpsBinWs w1, w2;                              // stage 1 over the clouds, stage 2 over the stage-1 points
    float* s1pos; int* s1idx;                     // (B, max_nobj, 3), (B, max_nobj): stage-1 points in selection order
    long long* off2; long long* n2;               // (B): where cloud b's stage-1 points start in s1pos, and how many
};
int fps_grid_cells_cap(int points, int cells);    // cells per cloud a pass over `points` points may use
size_t fps_grid_bytes();
size_t fps_grid_tab_bytes(int cells_cap);         // 0 where the tables fit LDS
hipError_t launch_fps_grid(const FpsGridArgs& a, hipStream_t st);

}  // namespace ag
