// mirhi_multiview.hip.h -- the batched entries of a multiview depth scope (mirhi_cmd_begin_rendering_multiview): the views of ONE scope share one
// vertex, one geometry and one raster launch, as the frames of a batched submit do (vertex_kernel_batch / geometry_kernel_batch / raster_kernel_batch).  Every
// view has parameters of its own (depth base = its layer; its own bins, counters, big list and vertex output), so the bodies are the single-view scope's,
// untouched: vertex_body<true>, geometry_body (through geometry_kernel_batch, which fits a depth-only scope as it is) and raster_body<0, KEYED, TP>.
// Included behind every older kernel: the code object keeps those in their order.
#ifndef MIRHI_MULTIVIEW_HIP_H
#define MIRHI_MULTIVIEW_HIP_H

// grid (waves of the vertex jobs, views): the jobs of all views are of one size (the same vertex ranges under another light matrix)
__global__ __launch_bounds__(GEOM_THREADS) void vertex_kernel_shadow_batch(const GeometryBatch B) { vertex_body<true>(B.params[blockIdx.y]); }

// grid (tiles_x, tile rows, views); KEYED / TP as raster_kernel_depth
template <int KEYED, int TP>
__global__ __launch_bounds__(RASTER_THREADS, (TP ? 7 : 8)) void raster_kernel_depth_batch(const RasterBatch B) {
    const uint32_t z = blockIdx.z;
    const RasterHead H = B.head[z];
    raster_body<0, KEYED, TP>(B.params[z], H);
}

#endif  // MIRHI_MULTIVIEW_HIP_H
