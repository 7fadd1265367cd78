// kmap_cells.h - what the kernel-map builders share: the kernel geometry (KernelGeom: centre rule, halo, lanes per row) and
// the block-hashed cell table (layout, block_id_of / cell_index lookups) of the binned builder (kmap_binned.hip), the probe
// kernel's cell lookup (kmap.hip), the strided layers (kmap_stride.hip) and the tally pass's duplicate repair (kmap_bucket.hip).
#pragma once

#include "wcn_common.h"

namespace wcn {

constexpr int kBlkShift = 3;
constexpr int kBlk = 1 << kBlkShift;    // 8 cells per axis
constexpr int kCells = kBlk * kBlk * kBlk;  // 512 row ids = 2 KB per occupied block
constexpr int kMaxHalo = 8;  // one block width: the 26 adjacent blocks still cover every probe
constexpr int kBlkCoordBits = kCoordBits - kBlkShift;  // 15-bit signed block coordinates
constexpr uint32_t kMaskUnwritten = 0x80000000u;       // top bit of a row's LAST mask word: no block has written the row
constexpr uint32_t kMaskDeferred = 0x80000001u;        // ... and its cell is not stored yet (block created by the 2nd insert pass)

// COMPACT neighbour rows (binned builder, one mask word, 17 <= K <= 31): 16 ints = 64 B per output row instead of 32 columns:
//   word 0 = the row's mask (bit k <=> offset k has a neighbour), words 1 .. popcount(mask) = the neighbour rows of the SET
//   offsets in ascending k, the rest unspecified.  Rows with more than kCompactIds neighbours do not fit: the builder raises
//   WCN_FLAG_ROW_OVERFLOW and the host rebuilds with dense rows.
constexpr int kCompactPitch = 16;
constexpr int kCompactIds = kCompactPitch - 1;
constexpr int kCompactFlag = (int)0x80000000;  // OR-ed into a `row pitch` kernel argument: the table is compact

constexpr int kIdLateBit = 1 << 30;  // set in a slot's id when the block was created by the SECOND insert pass

// block table slot: key 0 = empty; id = dense block id, valid for LATER launches than the one that created the block
struct __attribute__((aligned(16))) BSlot {
  uint64_t key;
  int32_t id;
  int32_t pad;
};

// The table is built in one of two modes, chosen on the device per build from the build's own coordinates:
//   hash    block ids are handed out in creation order by a counter (two insert passes, neighbour ids by hash lookups)
//   direct  the occupied 8^3 blocks fill their bounding box well enough (box_is_direct): a block's id is its linear index
//           in the box, every box block exists (the empty ones hold an all -1 sub-grid), neighbour ids are arithmetic
// Either way the hash slots hold (key, id) of every block, so block_id_of serves every other reader unchanged.
//
// ctr[64], cleared by cell_prepare:
constexpr int kCtrBlocks = 0;  // number of blocks (dense ids 0 .. ctr[0]-1; hash mode: may exceed max_blocks on overflow)
constexpr int kCtrMode = 1;    // 0 = hash, 1 = direct
constexpr int kCtrBox = 2;     // direct mode: [2..5] box origin, [6..9] box dims; block units, axes (batch, x, y, z)

constexpr int kDirectFill = 16;  // direct mode needs kDirectFill * box_blocks <= n: an average of 16 voxels per box block
constexpr int kBoxParts = 128;   // most partial bounding boxes cell_prepare writes (8 ints each)

// bounding box of the live voxels in block units, axes (batch, x >> 3, y >> 3, z >> 3)
struct BlockBox {
  int o[4];  // origin
  int d[4];  // dims (all 0: no live voxel)
};

__host__ __device__ inline BlockBox make_block_box(const int lo[4], const int hi[4]) {
  BlockBox b;
  const bool empty = lo[0] > hi[0];
  for (int a = 0; a < 4; ++a) {
    b.o[a] = empty ? 0 : lo[a];
    b.d[a] = empty ? 0 : hi[a] - lo[a] + 1;
  }
  return b;
}

__host__ __device__ inline int64_t box_blocks(const BlockBox& b) {
  return (int64_t)b.d[0] * b.d[1] * b.d[2] * b.d[3];  // <= 2^9 * 2^45
}

// Fill rule: at least kDirectFill voxels per box block on average (so box_blocks <= n / 16 <= the default max_blocks).
// Wrap rule: no spatial axis touches the ends of the signed block-coordinate range, so no neighbour key wraps.
__host__ __device__ inline bool box_is_direct(const BlockBox& b, int64_t n, int64_t max_blocks) {
  const int64_t blocks = box_blocks(b);
  if (blocks < 1 || blocks > max_blocks || blocks > n / kDirectFill) return false;
  const int lo = -(1 << (kBlkCoordBits - 1)), hi = (1 << (kBlkCoordBits - 1)) - 1;
  for (int a = 1; a < 4; ++a)
    if (b.o[a] <= lo || b.o[a] + b.d[a] - 1 >= hi) return false;
  return true;
}

// id of the box block at box-relative position r, or -1 outside the box
__host__ __device__ inline int box_block_id(const BlockBox& b, int r0, int r1, int r2, int r3) {
  if ((unsigned)r0 >= (unsigned)b.d[0] || (unsigned)r1 >= (unsigned)b.d[1] || (unsigned)r2 >= (unsigned)b.d[2] ||
      (unsigned)r3 >= (unsigned)b.d[3])
    return -1;
  return ((r0 * b.d[1] + r1) * b.d[2] + r2) * b.d[3] + r3;
}

// box-relative position of block id
__host__ __device__ inline void box_block_pos(const BlockBox& b, int id, int r[4]) {
  r[3] = id % b.d[3]; id /= b.d[3];
  r[2] = id % b.d[2]; id /= b.d[2];
  r[1] = id % b.d[1];
  r[0] = id / b.d[1];
}

__host__ __device__ inline uint64_t box_block_key(const BlockBox& b, const int r[4]) {
  return pack_key(b.o[0] + r[0], b.o[1] + r[1], b.o[2] + r[2], b.o[3] + r[3]);
}

struct CellTable {
  BSlot* slots;
  int64_t capacity;     // power of two >= 2 * max_blocks
  int32_t* ctr;         // counters and the build mode: kCtr* above
  int32_t* box;         // [kBoxParts][8] partial boxes of cell_prepare: min of (b, x, y, z), then min of the NEGATED (b, x, y, z)
  uint32_t* halo;       // halo gather list of the current kernel geometry
  uint64_t* blk_key;    // [max_blocks] dense id -> block key
  int32_t* nbtab;       // [max_blocks][32] ids of the 27 neighbour blocks (-1 = absent), [13] = the block itself
  int32_t* cells;       // [max_blocks][512] row ids, -1 = empty
  int64_t max_blocks;
  size_t bytes;
};

// kernel offset k = (i*ky + j)*kz + l  ->  (i - cx, j - cy, l - cz) * dilation; a probe's query is out * stride + offset
struct KernelGeom {
  int kx, ky, kz;  // kernel size
  int cx, cy, cz;  // centre
  int sx, sy, sz;  // stride
  int dx, dy, dz;  // dilation
};

// the centre rule: odd sizes are centred, even sizes start at the voxel itself
static inline KernelGeom make_kernel_geom(const int32_t ksize[3], const int32_t stride[3], const int32_t dilation[3]) {
  auto centre = [](int ks) { return (ks & 1) ? ks / 2 : 0; };
  return KernelGeom{ksize[0],  ksize[1],  ksize[2],  centre(ksize[0]), centre(ksize[1]), centre(ksize[2]),
                    stride[0], stride[1], stride[2], dilation[0],      dilation[1],      dilation[2]};
}

// max |offset| along one axis
static inline int kernel_halo(int ks, int c, int d) {
  const int lo = c * d, hi = (ks - 1 - c) * d;
  return lo > hi ? lo : hi;
}

// lanes of a wave that share one table row in the one-lane-per-(row, offset) kernels: 8, 16, 32 or 64
static inline int lanes_per_row(int kp) {
  int l = 8;
  while (l < kp && l < 64) l <<= 1;
  return l;
}

struct CellGeom {
  int kx, ky, kz, cx, cy, cz, dx, dy, dz;  // of the KernelGeom (stride 1)
  int hx, hy, hz;   // halo per axis (max |offset|)
  int px, py;       // LDS grid pitches (x, y); z pitch 1
  int cells;        // LDS grid size in ints
  int halo_cells;   // entries of the halo gather list
};

static inline int64_t cell_capacity(int64_t max_blocks) {
  int64_t c = 1024;
  while (c < 2 * max_blocks) c <<= 1;
  return c;
}

static inline CellTable carve_cells(void* ws, int64_t n, int64_t max_blocks) {
  CellTable t;
  char* p = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += align256(bytes); return q; };
  (void)n;
  t.max_blocks = max_blocks;
  t.capacity = cell_capacity(max_blocks);
  t.ctr = (int32_t*)take(256);
  t.box = (int32_t*)take((size_t)kBoxParts * 8 * 4);
  t.halo = (uint32_t*)take((size_t)16384 * 4);  // (8 + 2*8)^3 - 512 = 13312 entries at most
  t.slots = (BSlot*)take((size_t)t.capacity * sizeof(BSlot));
  t.blk_key = (uint64_t*)take((size_t)max_blocks * 8);
  t.nbtab = (int32_t*)take((size_t)max_blocks * 32 * 4);
  t.cells = (int32_t*)take((size_t)max_blocks * kCells * 4);
  t.bytes = off;
  return t;
}

static inline CellGeom make_cell_geom(const int32_t ksize[3], const int32_t dilation[3]) {
  const int32_t unit[3] = {1, 1, 1};
  const KernelGeom k = make_kernel_geom(ksize, unit, dilation);
  CellGeom g;
  g.kx = k.kx; g.ky = k.ky; g.kz = k.kz;
  g.cx = k.cx; g.cy = k.cy; g.cz = k.cz;
  g.dx = k.dx; g.dy = k.dy; g.dz = k.dz;
  g.hx = kernel_halo(g.kx, g.cx, g.dx); g.hy = kernel_halo(g.ky, g.cy, g.dy); g.hz = kernel_halo(g.kz, g.cz, g.dz);
  const int gx = kBlk + 2 * g.hx, gy = kBlk + 2 * g.hy, gz = kBlk + 2 * g.hz;
  // odd y pitch: the 27 cells a voxel probes then fall into 27 different LDS banks for a 3x3x3 kernel (pitches 11, 110)
  g.py = gz | 1;
  g.px = gy * g.py;
  g.cells = gx * g.px;
  g.halo_cells = gx * gy * gz - kCells;
  return g;
}

// slot of an existing block key, or -1
__device__ __forceinline__ int block_find(const BSlot* __restrict__ slots, uint32_t cmask, uint64_t key) {
  uint32_t s = hash_slot(key, cmask);
  for (uint32_t a = 0; a <= cmask; ++a) {
    const uint64_t k = slots[s].key;
    if (k == 0ull) return -1;
    if (k == key) return (int)s;
    s = (s + 1) & cmask;
  }
  return -1;
}

// dense id of the block that holds voxel c = (b, x, y, z), or -1
__device__ __forceinline__ int block_id_of(const BSlot* __restrict__ slots, uint32_t cmask, const int4& c) {
  const int s = block_find(slots, cmask, pack_key(c.x, c.y >> kBlkShift, c.z >> kBlkShift, c.w >> kBlkShift));
  if (s < 0) return -1;
  const int id = slots[s].id;
  return id < 0 ? -1 : (id & ~kIdLateBit);
}

// cell inside a block's sub-grid: of block-relative coordinates (0 .. kBlk-1), of a voxel
__device__ __forceinline__ int cell_index(int x, int y, int z) { return (x * kBlk + y) * kBlk + z; }
__device__ __forceinline__ int cell_of(const int4& c) {
  return ((c.y & (kBlk - 1)) * kBlk + (c.z & (kBlk - 1))) * kBlk + (c.w & (kBlk - 1));
}

}  // namespace wcn
