/*
 * scsfm_mesh.h -- C ABI of libscsfm_mesh.so: an indexed triangle mesh of the surface in a fused volume (the TSDF volume of
 * include/scsfm_fuse.h) by marching tetrahedra on the voxel grid, as hand-written HIP kernels for gfx950 (MI355X).
 *
 * Conventions (as include/scsfm_fuse.h)
 *  - All pointers are DEVICE pointers; the caller owns every buffer; nothing is retained.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no call synchronises or allocates.
 *  - Return value: 0 on success, SCSFM_MESH_ERR_ARG (-1) for a rejected argument (before any pointer is touched),
 *    otherwise the hipError_t of the failed launch.  The size function returns 0 for a rejected argument.  Every output
 *    is stored (overwritten), never accumulated.
 *  - No float atomics and no atomics at all: vertices and triangles are placed by integer scans, so the result is
 *    bit-identical from run to run.
 *
 * Volume.  As include/scsfm_fuse.h: nx x ny x nz voxels, x fastest (voxel (x, y, z) has the linear index
 * (z ny + y) nx + x), nvox = nx ny nz <= 2^29, five fp32 planes of nvox each: tsdf (t), weight (w), r, g, b.  The centre
 * of voxel i on an axis with origin o and voxel size s is  fl(o + fl(fl(float(i) + 0.5f) s)).  A voxel is SEEN when
 * w >= min_weight and NEGATIVE when t < 0 (a NaN and -0.0 are not).
 *
 * Arithmetic.  fp32, one rounding per operation (no fused multiply-add), `/` correctly rounded, denormals kept.
 *
 * Cells and corners.  A cell is the cube of the eight voxel centres (x + dx, y + dy, z + dz) for 0 <= x < nx - 1 and
 * likewise in y and z; its linear index is that of its minimum voxel.  Corner k has dx = k & 1, dy = (k >> 1) & 1,
 * dz = k >> 2.  A volume with a size of 1 has no cell.
 *
 * Tetrahedra.  Every cell is split into Kuhn's six tetrahedra round the diagonal 0-7, in this order of corner lists:
 *   0: (0,1,3,7)   1: (0,1,5,7)   2: (0,2,3,7)   3: (0,2,6,7)   4: (0,4,5,7)   5: (0,4,6,7)
 * The split is the same in every cell, so neighbouring cells agree on every face diagonal and the surface has no cracks.
 *
 * Edges.  A cell has 19 edges.  Voxel a owns the seven that start at it, by type e = 0 .. 6 with b = a + offset(e):
 *   e:      0      1      2      3      4      5      6
 *   offset: +x     +y     +z     +x+y   +x+z   +y+z   +x+y+z
 * (an edge between corners p < q of a tetrahedron always has the bits of p among those of q: its owner is the voxel at
 * corner p and its offset is corner q - p).  The cell's other twelve edges belong to its neighbours.
 *
 * Vertices.  One per crossing edge.  The edge from a to b = a + offset(e), b inside the volume, is a crossing when
 *   a and b are seen  &&  (t_a < 0) != (t_b < 0).
 * Then
 *   frac = t_a / fl(t_a - t_b)
 *   every coordinate in which a and b differ is fl(c_a + fl(frac voxel)), c_a a's centre; the others are a's centre;
 *   a coordinate that comes out as a NaN (a NaN or infinite t) is stored as the quiet NaN 0x7fc00000, whatever sign
 *   and payload the hardware's division left
 *   colour = fl(col_a + fl(frac fl(col_b - col_a))) per channel, c = colour >= 0 ? colour : 0 (a NaN becomes 0),
 *   c = c <= 1 ? c : 1, byte = uint8(fl(fl(c 255.0f) + 0.5f))
 * exactly as include/scsfm_fuse.h's extraction.  Vertex order: by the linear index of a, then by e.  The vertices with
 * e < 3, taken in order, are therefore what scsfm_fuse_extract writes, bit for bit (but for the sign and payload of a NaN
 * coordinate, which that library leaves as the hardware gives them).  A vertex that no triangle uses can
 * occur at the rim of the seen region (its edge crosses, but no tetrahedron round it has four seen corners); it is
 * kept: the vertex list is a pure function of the edges.
 *
 * Triangles.  A tetrahedron emits triangles only if all four of its corners are seen.  Let I be its negative corners
 * and O the others, both in the order of its corner list.
 *   |I| = 0 or 4: nothing.
 *   |I| = 1: one triangle on the edges (I0,O0), (I0,O1), (I0,O2).
 *   |I| = 3: one triangle on (I0,O0), (I1,O0), (I2,O0).
 *   |I| = 2: the quadrilateral q0 .. q3 on (I0,O0), (I0,O1), (I1,O1), (I1,O0), as the triangles (q0,q1,q2), (q0,q2,q3).
 * Every edge named here has a sign change between two seen voxels, so it is a crossing and has a vertex.
 * Orientation: a triangle (A, B, C) runs counter-clockwise seen from the non-negative side, that is, (B - A) x (C - A)
 * points from the I corners to the O corners (towards free space and the cameras).  Where the order above runs the
 * other way, the triangle's last two indices are swapped.  Whether it does depends only on the tetrahedron and on the
 * 4-bit case (bit j set: corner j of the corner list is negative), not on the fractions.  Bit c of
 *   SCSFM_MESH_FLIP(tetrahedron) = 0x4d24 for the tetrahedra 0, 3, 4,  0x32da for 1, 2, 5
 * is set when case c is swapped (both triangles of a quadrilateral alike).
 * Triangle order: by the cell's linear index, then the tetrahedron 0 .. 5, then the first and the second triangle.
 * A triangle is three int32 indices into the vertex list.  Degenerate triangles (a fraction of exactly 0 or 1) are
 * kept; nothing is culled, welded or smoothed.
 *
 * Workspace (scsfm_mesh_ws_bytes; C = ceil(nvox / SCSFM_MESH_CHUNK) chunks of consecutive voxels):
 *   2 x int64   the number of vertices V, the number of triangles T     (the host reads these 16 bytes once)
 *   C x int32   the vertices owned by the voxels of every chunk;  C x int32  the triangles of its cells
 *   C x int64   the exclusive scan of the first;                  C x int64  of the second
 *   nvox x int32  the index of every voxel's first vertex         (written by scsfm_mesh_vertices)
 *   nvox x uint8  the voxel's 7-bit crossing mask, bit e          (written by scsfm_mesh_vertices)
 * The index of the vertex of edge (a, e) is a's first index plus the number of set bits of a's mask below bit e: the
 * triangle pass looks an index up with two loads and searches nothing.  That is 5 bytes a voxel beside the volume's 20.
 */
#ifndef SCSFM_MESH_H_
#define SCSFM_MESH_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCSFM_MESH_ERR_ARG (-1)
#define SCSFM_MESH_MAX_VOXELS (1 << 29)
#define SCSFM_MESH_CHUNK 1024    /* consecutive voxels (by linear index) per chunk */
#define SCSFM_MESH_FLIP(tet) ((0x26 >> (tet)) & 1 ? 0x32da : 0x4d24)

/* 1 (first version) */
int scsfm_mesh_abi_version(void);
/* the source id of the build (scsfm_hip/build.py: mesh_source_id) into buf, NUL-terminated */
int scsfm_mesh_source_id(char* buf, size_t n);

/* bytes of the workspace (see above); 0 for a rejected argument (a size <= 0, nvox > 2^29) */
size_t scsfm_mesh_ws_bytes(int nx, int ny, int nz);

/* Counts the vertices and the triangles of every chunk, scans both and stores the totals, all into ws (16-byte
   aligned, ws_bytes >= scsfm_mesh_ws_bytes).  Reads the tsdf and weight planes only.  min_weight >= 1. */
int scsfm_mesh_count(int nx, int ny, int nz, const float* volume, float min_weight, void* ws, size_t ws_bytes,
                     void* stream);

/* Writes the vertices in their order: vertex k < capacity to xyz[k, 3] and rgb[k, 3]; nothing at or past capacity
   (0: xyz and rgb may be NULL).  Also records every voxel's first index and mask in ws, whatever the capacity.  ws is
   what scsfm_mesh_count left for the same volume and min_weight, n_vertices the total the host read from it: one above
   2^31 - 1 is refused (-1), never wrapped (and a total in ws above it makes the kernel write nothing). */
int scsfm_mesh_vertices(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* volume,
                        float min_weight, void* ws, size_t ws_bytes, size_t n_vertices, int capacity, float* xyz,
                        unsigned char* rgb, void* stream);

/* Writes the triangles in their order: triangle k < capacity to tri[k, 3]; nothing at or past capacity (0: tri may be
   NULL, and nothing is launched).  ws is what scsfm_mesh_count and scsfm_mesh_vertices left for the same volume and
   min_weight; n_vertices and n_triangles are the totals the host read from it: either above 2^31 - 1 is refused. */
int scsfm_mesh_triangles(int nx, int ny, int nz, const float* volume, float min_weight, const void* ws, size_t ws_bytes,
                         size_t n_vertices, size_t n_triangles, int capacity, int* tri, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCSFM_MESH_H_ */
