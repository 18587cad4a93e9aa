// The tile table: every block-tile configuration of the GEMM kernels, described ONCE.  Host-side constexpr, no device code.
//   * gemm.hip generates its TileCfg instantiations and the variant dispatch from TILES (CfgAt<index>, by_variant) and asserts the derived
//     values below against the kernel's own TileCfg::LDS / NT;
//   * tile_rules.hip prices and aligns the tiles a rule returns from the same rows (tile2_dims, tile_bm, mlp_gemm_cost, pick_gemm8_tile);
//   * the 8-phase kernels' three tiles (gemm8.hip / gemm8f.hip, ids 16-18) are TILES8.
// Adding or retiring a tile is one row here.  tests/test_host_logic.py keeps its own hand-written tables: the independent statement this one is
// checked against.
#pragma once

namespace vp {

// id = GemmArgs::variant.  product: instantiated in the product library (the ids a rule of tile_rules.hip can return); every row is instantiated in the
// measurement build (-DVP_TOOLS).  partial: instantiated for EPI_PARTIAL (the tiles pick_splitk may name for the split-K partial products).
struct TileRow {
    int id, BM, BN, BK, WM, WN, STAGES, PIPE;
    bool product, partial;
};

// PIPE = the k-step schedule: 0 plain, 1 the fragment reads of k-half 1 issued inside the MFMAs of k-half 0, 6 two k-blocks per barrier.
// Measured on MI355X at M = 49152 (tools/gemm_tune.py, profiles/gemm_tune_r1.txt).  Default = id 8: one 192-token crop per m-tile, so the tile count divides
// evenly over 256 CUs x 2 resident blocks for every encoder GEMM (no tail wave), and the epilogue of one block overlaps the main loop of its CU partner.
// 256x256 halves the L2->LDS operand traffic but runs 1 block / CU (epilogue exposed, tail wave at N = D).
// id 11 = the id 8 block tile cut into 8 wave tiles of 48x64: same main-loop rate (LDS reads are at 18 % utilisation, so the smaller wave tile costs
// nothing), but twice the threads for the VALU-heavy residual epilogue (plane split + LayerNorm statistics): proj+fc2 4.54 -> 4.30 ms per step; no gain
// for qkv / fc1, slower for the deconvs (96x32 wave tiles: -25 %).
// Ids 4, 5, 6 and 10 are retired: register double-buffered fragments (PIPE 2), fragment-shaped epilogue stores, the staggered two-group schedule (PIPE 3)
// and hand-scheduled ds_reads with counted lgkmcnt (PIPE 5) all lost; their code can be read from commit a3d3210.
// The trailing columns of the comments (ring KiB, waves, blocks / CU) are what tile_ring_bytes / tile_threads / tile_wgs_per_cu below compute.
inline constexpr TileRow TILES[] = {
    // id   BM   BN  BK   WM  WN ST PIPE product partial
    {0, 128, 128, 64, 64, 64, 2, 0, false, false},    //  64 KiB   4   (2 blocks / CU)
    {1, 128, 128, 64, 64, 64, 2, 1, true, true},      //  same + pipelined fragment reads
    {2, 256, 256, 64, 128, 64, 2, 0, false, false},   // 128 KiB   8   (1 block / CU)
    {3, 256, 256, 64, 128, 64, 2, 1, true, false},    //  same + pipelined fragment reads
    {7, 192, 256, 64, 96, 64, 2, 1, false, false},    // 112 KiB   8   (1 block / CU)
    {8, 192, 128, 64, 96, 64, 2, 1, true, false},     //  80 KiB   4   (2 blocks / CU)  <- default
    {9, 64, 64, 64, 32, 32, 2, 0, true, false},       //  32 KiB   4   (5 blocks / CU)  small batches: enough tiles to fill 256 CUs
    {11, 192, 128, 64, 48, 64, 2, 1, true, true},     //  80 KiB   8   id 8 tile as 8 waves of 48x64 (4 waves / SIMD, 122 VGPRs)  <- default for the residual GEMMs
    // small batches (a few crops per GPU): the 2-stage ring waits for every k-block's full L2 latency; deeper rings keep 2-3 blocks in flight
    {12, 64, 64, 64, 32, 32, 4, 0, true, true},       //  64 KiB   4   (2 blocks / CU)  id 9 with a 4-stage ring
    {13, 128, 128, 64, 64, 64, 3, 1, false, false},   //  96 KiB   4   (1 block / CU)   id 1 with a 3-stage ring
    {14, 64, 64, 64, 32, 32, 3, 0, false, false},     //  48 KiB   4   (3 blocks / CU)  id 9 with a 3-stage ring
    {15, 128, 64, 64, 64, 32, 3, 0, true, true},      //  72 KiB   4   (2 blocks / CU)  128(m) x 64(n), 3-stage ring
    // (16-18 = the 8-phase kernel: TILES8 below.)  Round 5, small batches IN SITU: every layer's weights are first touched from HBM (ViTPose-L: 25 MB per layer,
    // 600 MB per forward -- more than L2 + the memory-side cache hold), so a k-block costs an HBM round trip, not the L2 hit the isolated sweeps of rounds 2-3 saw:
    // a workgroup retires STAGES - 1 k-blocks per round trip whatever its tile, and one full round of workgroups with a deep ring beats more, smaller tiles.
    {19, 192, 128, 64, 96, 64, 3, 1, false, false},   // 120 KiB   4   (1 block / CU)   id 8 with a 3-stage ring
    {20, 192, 128, 64, 48, 64, 3, 1, true, true},     // 120 KiB   8   (1 block / CU)   id 11 with a 3-stage ring
    {21, 64, 64, 64, 32, 32, 5, 0, false, false},     //  80 KiB   4   (2 blocks / CU)  id 9 with a 5-stage ring
    {22, 128, 64, 64, 64, 32, 6, 0, false, false},    // 144 KiB   4   (1 block / CU)   128(m) x 64(n), 6-stage ring
    {23, 64, 64, 64, 32, 32, 8, 0, false, false},     // 128 KiB   4   (1 block / CU)   id 9 with an 8-stage ring
    {24, 128, 128, 64, 64, 64, 4, 1, false, false},   // 128 KiB   4   (1 block / CU)   id 1 with a 4-stage ring
    {25, 128, 128, 32, 64, 64, 4, 0, false, false},   //  64 KiB   4   (2 blocks / CU)  128 x 128 with k-blocks of 32: 4-stage ring in id 1's LDS
    {26, 128, 128, 32, 64, 64, 5, 0, false, false},   //  80 KiB   4   (2 blocks / CU)  ... 5-stage
    {27, 64, 64, 64, 32, 32, 4, 1, false, false},     //  64 KiB   4   (2 blocks / CU)  id 12 with pipelined fragment reads
    {28, 64, 64, 64, 32, 32, 5, 6, false, false},     //  80 KiB   4   (2 blocks / CU)  64 x 64, two k-blocks per barrier, 5-stage ring (3 k-blocks in flight)
    {29, 64, 64, 64, 32, 32, 4, 6, false, false},     //  64 KiB   4   (2 blocks / CU)  ... 4-stage ring (2 in flight)
    {30, 64, 64, 64, 32, 32, 6, 6, true, true},       //  96 KiB   4   (1 block / CU)   ... 6-stage ring (4 in flight)
    {31, 32, 64, 64, 16, 32, 6, 6, true, true},       //  72 KiB   4   (2 blocks / CU)  32(m) x 64(n): twice the workgroups of a 1-2 crop GEMM, half the MFMAs per wave and k-block
    {32, 32, 64, 64, 16, 32, 8, 6, false, false},     //  96 KiB   4   (1 block / CU)   ... 8-stage ring (6 in flight)
    {41, 96, 64, 64, 48, 32, 4, 0, true, false},      //  80 KiB   4   (2 blocks / CU)  96(m) x 64(n), 4-stage ring: the residual GEMMs between the 64 x 64 and 128 x 64 regimes (round 6: <= 448 tiles;
                                                      //                                 ViTPose-L 11-14 crops, -B 15-18, -H 9-11: profiles/small_batch_r6.txt call 18)
};
// (round 6, measured and not kept -- profiles/small_batch_r6.txt calls 13, 15: a 4-stage ring on the one-round 192 x 128 tile (+1 %), the 96 x 64 tile with a 6-stage ring /
// two k-blocks per barrier (loses wherever the 4-stage one wins).)
inline constexpr int NUM_TILES = (int)(sizeof(TILES) / sizeof(TILES[0]));

// the row of an id, or nullptr
constexpr const TileRow* find_tile(int id) {
    for (int i = 0; i < NUM_TILES; ++i)
        if (TILES[i].id == id) return &TILES[i];
    return nullptr;
}

// Derived values.  The kernel's TileCfg::LDS / NT stay the authority: gemm.hip asserts these formulas against them for every row.
constexpr int LDS_PER_CU = 160 * 1024, NUM_CUS = 256;
constexpr int tile_ring_bytes(const TileRow& r) { return r.STAGES * (r.BM + r.BN) * r.BK * 2; }   // STAGES x (A tile + W tile) of 16-bit operands
constexpr int tile_threads(const TileRow& r) { return (r.BM / r.WM) * (r.BN / r.WN) * 64; }
constexpr int tile_wgs_per_cu(const TileRow& r) { return LDS_PER_CU / tile_ring_bytes(r); }       // resident workgroups per CU
constexpr int tile_slots(const TileRow& r) { return NUM_CUS * tile_wgs_per_cu(r); }               // ... on the chip

// The 8-phase persistent kernels (gemm8.hip, gemm8f.hip): one 512-thread workgroup per CU
struct Tile8Row { int id, BM, BN; };
inline constexpr Tile8Row TILES8[] = {{16, 256, 256}, {17, 256, 192}, {18, 192, 256}};
constexpr const Tile8Row* find_tile8(int id) {
    for (const Tile8Row& r : TILES8)
        if (r.id == id) return &r;
    return nullptr;
}
constexpr bool is_gemm8(int id) { return find_tile8(id) != nullptr; }
constexpr int tile8_bm(int id) { return find_tile8(id) ? find_tile8(id)->BM : 0; }
constexpr int tile8_bn(int id) { return find_tile8(id) ? find_tile8(id)->BN : 0; }

// May the LayerNorm CONSUMER running on this tile fold the producer's partial statistics itself beyond the small-batch threshold (tile_rules.hip plan_chunk)?
// Measured (profiles/small_batch_r6.txt call 25): the (mean, rstd) area behind the ring costs the 80 KiB ring of the default 192 x 128 tile its second
// workgroup per CU, so ids 8 and 11 do not fold; the 8-phase kernel reads finished row statistics.  This is a LIST OF MEASURED CASES, not the derivation
// "does the area change LDS_PER_CU / ring": that derivation would also exclude id 9 (5 -> 4 workgroups per CU) and id 41 (2 -> 1), which fold today.
constexpr bool tile_folds_stats(int id) { return id != 8 && id != 11 && !is_gemm8(id); }

// what tile_rules.hip priced its rules with: the slots of the eleven product tiles
constexpr bool tile_slots_are(int id, int slots) { return find_tile(id) && find_tile(id)->product && tile_slots(*find_tile(id)) == slots; }
static_assert(tile_slots_are(8, 512) && tile_slots_are(11, 512) && tile_slots_are(3, 256) && tile_slots_are(9, 1280) && tile_slots_are(12, 512) && tile_slots_are(15, 512) &&
              tile_slots_are(1, 512) && tile_slots_are(20, 256) && tile_slots_are(30, 256) && tile_slots_are(31, 512) && tile_slots_are(41, 512), "resident slots of the product tiles");

}  // namespace vp
