// Host-side planning of the entries that export meshes into the handle's scratch a batch of frames at a time
// (moshii_virtual_markers_*, moshii_marker_surface_distance_*): the batch length and the scratch layout.  Pure arithmetic -- C++17 and
// standard headers only, no HIP types, no environment -- so that it is tested on its own (tests/test_export_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>

namespace export_plan {

constexpr size_t kMeshBudget = (size_t)256 << 20;   // bytes of meshes in flight
constexpr long long kFrameTile = 128;               // the f32 export works in tiles of this many frames
constexpr long long kGridY = 65535;                 // the f64 export puts the frames on grid.y

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct Batch {
    long long batch = 0;                              // frames per batch
    // moshii_virtual_markers_*: [meshes of a batch | items marker vertex ids (int) | items distances (double)]
    size_t off_vids = 0, off_dist = 0, vm_bytes = 0;
    // moshii_marker_surface_distance_*: [meshes of a batch | batch x items winners (int), unless the caller takes `face`]
    size_t off_win = 0, sd_bytes_face = 0, sd_bytes = 0;
};

// frame_bytes: one mesh; F >= 1 frames; items >= 1: markers (M) or points (N) per frame; override_batch: MOSHII_VM_BATCH, 0 = unset.
// Frames per batch: 256 MB of meshes (SMPL-H, 82 680 bytes a frame in f32: 3 246 frames, 3 200 in whole tiles; f64: 1 623, 1 536),
// whole 128-frame tiles where it reaches one; no more than F; batch x items fits an int; f64: no more than grid.y takes.
inline Batch plan_batch(size_t frame_bytes, long long F, long long items, bool is_f64, int override_batch) {
    Batch b;
    long long batch = std::max<long long>(1, (long long)kMeshBudget / (long long)frame_bytes);
    if (batch >= kFrameTile) batch = batch / kFrameTile * kFrameTile;
    if (override_batch > 0) batch = override_batch;   // (tests: batch boundaries with few frames)
    batch = std::min<long long>(std::min<long long>(batch, F), 0x7fffffffLL / items);
    if (is_f64) batch = std::min<long long>(batch, kGridY);
    b.batch = batch;
    b.off_vids = b.off_win = align16((size_t)batch * frame_bytes);
    b.off_dist = align16(b.off_vids + (size_t)items * sizeof(int));
    b.vm_bytes = b.off_dist + (size_t)items * sizeof(double);
    b.sd_bytes_face = b.off_win;
    b.sd_bytes = b.off_win + (size_t)batch * (size_t)items * sizeof(int);
    return b;
}

// moshii_render_* / moshii_render_posed_*: a batch of frames is rendered from
//   [meshes of a batch (posed call only) | their vertex normals | V projected records a frame | N marker records a frame |
//    the cameras | N radii (double) | N colours (3 bytes)]
// every part on a 16-byte boundary.  The cameras, radii and colours are the call's, not the batch's.
struct RenderBatch {
    long long batch = 0;
    size_t off_normals = 0, off_rec = 0, off_mrec = 0, off_cams = 0, off_radius = 0, off_prgb = 0, bytes = 0;
};
constexpr size_t kRenderVertexBytes = 32, kRenderMarkerBytes = 40, kCameraBytes = 17 * sizeof(double);

// frame_bytes: one mesh (= one frame of normals); F >= 1 frames of V vertices and N >= 0 points, n_cameras cameras; posed: the meshes
// are exported into the scratch as well; override_batch: MOSHII_VM_BATCH, 0 = unset.
// Frames per batch: 256 MB of meshes, normals and records; whole 128-frame tiles where it reaches one; no more than F; no more than
// 65 535 (the frames of a batch are the tile kernel's grid.z and the f64 export's grid.y).
inline RenderBatch plan_render(size_t frame_bytes, long long F, long long V, long long N, long long n_cameras, bool posed, int override_batch) {
    RenderBatch b;
    const size_t per_frame = (posed ? 2 : 1) * frame_bytes + (size_t)V * kRenderVertexBytes + (size_t)N * kRenderMarkerBytes;
    long long batch = std::max<long long>(1, (long long)(kMeshBudget / per_frame));
    if (batch >= kFrameTile) batch = batch / kFrameTile * kFrameTile;
    if (override_batch > 0) batch = override_batch;
    batch = std::min<long long>(std::min<long long>(batch, F), kGridY);
    b.batch = batch;
    b.off_normals = posed ? align16((size_t)batch * frame_bytes) : 0;
    b.off_rec = align16(b.off_normals + (size_t)batch * frame_bytes);
    b.off_mrec = align16(b.off_rec + (size_t)batch * (size_t)V * kRenderVertexBytes);
    b.off_cams = align16(b.off_mrec + (size_t)batch * (size_t)N * kRenderMarkerBytes);
    b.off_radius = align16(b.off_cams + (size_t)n_cameras * kCameraBytes);
    b.off_prgb = align16(b.off_radius + (size_t)N * sizeof(double));
    b.bytes = b.off_prgb + (size_t)N * 3;
    return b;
}

}  // namespace export_plan
