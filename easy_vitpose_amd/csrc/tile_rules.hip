// Tile rules: which kernel runs each GEMM of a chunk -- pure host functions of the switches and the shape (no device, no handle).  The single rules
// (pick_*) feed one resolver per GEMM (resolve_gemm) and one plan per chunk (plan_chunk), which the orchestration (forward.hip) only executes.
// tests/test_host_logic.py walks the rules and the plan over every batch size of every model through the host-only taps at the end of this file.
#include "api_internal.h"
#include "hoststage.h"
#include "tiles.h"

using namespace vpi;

namespace vpi {

struct G8Pick { int variant, bm, bn; long tiles; };
struct Tile2Pick { int variant, group_m; };
using vp::is_gemm8;
struct SplitKPick { int S, variant; };   // split-K of a residual GEMM: S k ranges on tile configuration `variant` (S = 1: no split)

// Tile of the 8-phase kernel for an [M, N] output (wide = 16-bit output, else residual epilogue); variant 0 = the 2-phase kernels run it.
// A pure function of the shape: tests/test_host_logic.py walks it over every batch size through the host-only tap vp_dbg_gemm8_pick.
//
// A candidate QUALIFIES (round 3, measured in situ at batch 32 - 256: ViTPose-B qkv at 216 / 432 tiles -15 % / -5 %, fc2 at 216 tiles -23 %, but
// fc1 / fc2 at 288 tiles = 56 % full +20 %; ViTPose-H fc2 at batch 128, 480 tiles: 329 -> 279 us) from 1.75 tiles per CU (448), or from 192 tiles
// when its last round is >= 80 % full.  Round 4 (`extended`; profiles/tile_sweep_r4.txt: isolated sweep + in-situ A/B at 40 - 256 crops) adds, from
// 7 680 rows on: a launch of ONE round from 192 tiles (fc2 at 88 crops: 198 tiles of 256 x 256, 110 -> 87 us), and a candidate whose
// rounds x tile area is below the 2-phase kernel's rounds x work of a CU per round (two 192 x 128 workgroups per CU; one when <= 256 tiles) --
// fc2 at 172 crops: 387 tiles of 256 x 256 = 2 rounds against 3 rounds of everything else, 200 -> 173 us.  Among the qualifying candidates the
// cheapest rounds x area wins (192 x 256 priced x 1.08: measured 1 - 8 % behind 256 x 192 at equal rounds; ties: the larger tile); without
// `extended` the 192 x 256 tile is only the fallback when no 256-row tile qualifies.  Where isolated and in-situ timings disagreed (fc2 at 52 / 128
// crops, ViTPose-L at 40, -S at 256: the 2-phase kernel finds `hid` in the caches and wins by 2 - 7 % in situ) the rule follows the in-situ result.
G8Pick pick_gemm8_tile(int M, int N, bool wide, int bm192_mask, long min_tiles, bool extended) {
    const bool ext = extended && M >= 7680;
    const long t2 = (long)((M + 191) / 192) * ((N + 127) / 128);
    const double cost2 = t2 <= 256 ? 24576.0 : (double)((t2 + 511) / 512) * 49152.0;
    G8Pick pk{0, 0, 0, 0};
    double best = 0.0;
    bool have256 = false;
    for (const vp::Tile8Row& cd : vp::TILES8) {   // in table order: 256 x 256, 256 x 192, 192 x 256
        if (M % cd.BM || N % cd.BN || (wide && cd.id == 17)) continue;
        if (cd.id == 18 && (!(bm192_mask & (wide ? 2 : 1)) || (!ext && have256))) continue;   // round-3 behaviour: only when no 256-row tile qualifies
        const long t = (long)(M / cd.BM) * (N / cd.BN);
        if (t < 8) continue;
        const long rounds = (t + 255) / 256;
        const double f = (double)t / (double)(rounds * 256);   // share of 256 CUs x rounds that computes a tile (below 256 tiles: one workgroup per tile)
        const double cost = (double)rounds * cd.BM * cd.BN * (cd.id == 18 ? 1.08 : 1.0);
        bool q = t >= min_tiles || (f >= 0.8 && t >= 192);
        if (ext) q = q || (rounds == 1 && t >= 192) || cost < 0.95 * cost2;
        if (!q) continue;
        if (cd.BM == 256) have256 = true;
        if (!pk.variant || (ext ? cost < 0.98 * best : f > (double)pk.tiles / (double)up256((size_t)pk.tiles) + 1e-9)) {
            pk = {cd.id, cd.BM, cd.BN, t};
            best = cost;
        }
    }
    return pk;
}

// Tile configuration of the 2-phase kernel (gemm.hip Cfg id) for one GEMM of the path -- a pure function of the epilogue and the shape: tests/test_host_logic.py
// walks it over every batch size of every model through the host-only tap vp_dbg_gemm2_pick (slots, rounds, the PIPE-6 precondition, the measured choices).
//
// Default: the 192(m) x 128(n) tile -- M is always a multiple of 192 tokens (one crop per m-tile), so the tile count divides evenly over 256 CUs x 2 workgroups at
// the BASELINE batch; best or tied for every encoder GEMM in the MI355X sweep (profiles/gemm_tune_r1.txt); residual GEMMs: the same tile as 8 waves; wide GEMMs use
// the grouped order.  Small batches (fewer than 384 such tiles, e.g. 8 crops per GPU of a sharded frame): tiles that still give the 256 CUs a workgroup each --
// 128 x 128 from 256 tiles on, else 64 x 64, and inside the 64 x 64 regime (round 5, measured IN SITU: tools/small_sweep.py, profiles/small_batch_r5.txt):
//   64 x 64 tiles are bound by the latency of every k-block (a workgroup retires STAGES - 1 k-blocks per round trip) and, with one workgroup per SIMD set, by the
//   ~500 cycles of wait + barrier + LDS round trip in front of the 8 MFMAs of a k-step.  Inside the step every layer's weights are first touched from HBM, so the round
//   trip is ~2 x what the isolated sweeps of rounds 2-3 (weights L2-resident) saw.  Every choice keeps the k order: bit-identical.
//   * <= 256 tiles of 32 x 64: Cfg31 = 32(m) x 64(n) tiles, 6-stage ring, TWO k-blocks per barrier (gemm.hip PIPE 6) -- twice the workgroups, half the MFMAs per wave
//     and k-block;  <= 256 tiles of 64 x 64: Cfg30 = that schedule on 64 x 64 tiles, one workgroup per CU;
//   * <= 512 tiles (all resident at the 2 workgroups per CU of the 4-stage ring): Cfg12; more tiles would run the deep rings in two rounds and lose against the 5
//     workgroups per CU of the 2-stage ring (Cfg9) -- except for long K (round 2: Cfg12 from K = 2048 on);
//   * residual GEMMs (attn.proj, mlp.fc2) with more than 512 tiles of 64 x 64 but <= 512 of 128(m) x 64(n) (12-28 crops): Cfg15 = that tile on a 3-stage ring, all
//     resident at 2 workgroups per CU: fc2 of 16 crops 42 -> 34 us (-B), 56.5 -> 44 (-L), of 12 crops 72 -> 54 (-H).  For the wide GEMMs the same tile is neutral.
//   attn.proj of 1-8 crops 17-20 -> 10-13 us, mlp.fc2 of one crop 24.5 -> 17-21.5 us, qkv / fc1 of one crop 18 -> 12 us; ViTPose-L 1 crop 1.90 -> 1.36 ms, 8 crops
//   2.50 -> 2.40 ms, 16 crops 3.62 -> 3.23 ms; -B 1 crop 0.73 -> 0.56 ms, 16 crops 1.48 -> 1.33 ms; -H 1 crop 3.00 -> 2.17 ms, 12 crops 5.49 -> 4.81 ms.
Tile2Pick pick_gemm2_tile(int epi, int M, int N, int K) {
    Tile2Pick tp;
    tp.variant = (epi == vp::EPI_BIAS_RESID || epi == vp::EPI_BIAS_RESID_LN) ? 11 : 8;
    tp.group_m = (epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU) ? 8 : 0;
    const long par_ = (epi == vp::EPI_DECONV) ? 4 : 1;   // the four output parities of a deconv are four GEMMs of one launch
    const long t192 = (long)((M + 191) / 192) * ((N + 127) / 128) * par_;
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * par_;
    const bool wide = epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU;
    if (t192 >= 384) {
        // Round 6 (profiles/small_batch_r6.txt calls 18-21): more than 512 tiles of 192 x 128 are a second, mostly empty round of the 2 workgroups per CU.  Where the 8-phase
        // kernel has no tile for the row count (it takes the GEMM first, gemm()), every choice below keeps the k order (bit-identical):
        //   * <= 256 tiles of 256 x 256 (ragged last m-tile): ONE round of the 2-phase 256 x 256 tile (Cfg3).  Wide GEMMs: ViTPose-L 17-21 crops mlp.fc1 48.5 -> 38.5 us (step
        //     -9 ... -10.7 %), -B 22-27 crops -5 ... -7 %, -H 13-15 crops -5 ... -7.6 %, -S 43-55 crops -2 ... -3.6 %.  Residual GEMMs (57-85 crops of ViTPose-L, 86-113 of -B that are
        //     no multiple of 4): mlp.fc2 140 -> 116-139 us, step -2.3 ... -6.2 %; with 272 such tiles it loses (+20 %): the rule asks for one round;
        //   * else a wide GEMM whose 128 x 128 tiles still fit two rounds of the 512 slots (ViTPose-S attn.qkv at 57-75 crops: 25.0 -> 21-24 us, step -0.8 ... -3.1 %): 128 x 128.
        const bool enc = wide || epi == vp::EPI_BIAS_RESID_LN;
        if (enc && t192 > 512 && K >= 384 && K % 128 == 0 && N % 256 == 0 && (long)((M + 255) / 256) * (N / 256) <= 256) {
            tp.variant = 3;
            tp.group_m = wide ? 8 : 0;
        } else if (wide && t192 > 512 && t128 <= 1024) {
            tp.variant = 1;
            tp.group_m = 0;
        }
        return tp;
    }
    // Round 6: a wide GEMM whose 128 x 128 tiles need a second, mostly empty round (257-384 tiles on 256 CUs) while its 192 x 128 tiles are ONE round (<= 256: M is a
    // multiple of 192) runs on the 8-wave 192 x 128 tile with a 3-stage ring (Cfg20, one workgroup per CU) in groups of 8 m-tiles, m fastest (an XCD then owns a few
    // weight n-tiles x all crops).  K >= 1024 only: ViTPose-B's 12 k-blocks do not amortise the deeper prologue (measured +3 %, profiles/small_batch_r5.txt call 10).
    // ViTPose-L, 7-8 crops (one GPU's share of BASELINE configs[3]): qkv 25.6 -> 23.5 us, fc1 27.8 -> 25.5 us per layer; ViTPose-H at 8 crops: qkv only (fc1: 320 tiles).
    if ((epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU) && K >= 1024 && K % 128 == 0 && M % 192 == 0 && N % 128 == 0 && t128 > 256 && t192 <= 256) {
        tp.variant = 20;
        tp.group_m = 8;
        return tp;
    }
    // Round 6 (calls 18-19): 128 x 128 tiles beyond the 512 slots of 2 workgroups per CU while 192 x 128 tiles fit them: the default tile (ViTPose-L 11 crops fc1 37.9 -> 30.3 us,
    // -B 15 crops 31.8 -> 26.6, -S 40 crops qkv 20.8 -> 17.4; the residual GEMMs of ViTPose-L 43-47 / -B 58-63 / -H 35-38 crops: fc2 118 -> 92 / 95 -> 74 / 146 -> 114 us, step -11 %)
    if ((wide || epi == vp::EPI_BIAS_RESID_LN) && t128 > 512) return tp;
    const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64) * par_;
    const long t128x64 = (long)((M + 127) / 128) * ((N + 63) / 64) * par_;
    if (epi == vp::EPI_BIAS_RESID_LN && t64 > 512) {
        // residual GEMMs beyond the 512 resident 64 x 64 tiles (round 5: 128 x 64 on a 3-stage ring up to 512 tiles, then 128 x 128).  Round 6 (call 18, all bit-identical):
        //   * 96(m) x 64(n) tiles (Cfg41, 4-stage ring, 2 workgroups per CU) up to 448 of them: ViTPose-L 11-14 crops fc2 41-42 -> 36-38 us, proj 18.5 -> 16.4 (step -3.7 ... -4.9 %),
        //     -B 15-16 crops -4 ... -5.6 %; at 480-512 tiles it loses (-L 16 crops 44 -> 49 us, -B 20 crops +1.8 %);
        //   * beyond 512 tiles of 128 x 64 the 128 x 128 tile ran one workgroup per CU on a 2-stage ring (fc2 of ViTPose-L 21-32 crops flat at 66-72 us): the 8-wave 192 x 128 tile
        //     on a 3-stage ring (Cfg20), one round of <= 256 tiles, 60-64 us, proj 27-29.5 -> 25-27: ViTPose-L 24 / 28 / 32 crops -5.5 / -5.6 / -4.9 %, -B 29 / 32 / 34 crops -4.9 / -4.5 / -4.9 %.
        const long t96x64 = (long)((M + 95) / 96) * ((N + 63) / 64);
        tp.group_m = 0;
        tp.variant = t96x64 <= 448 ? 41 : t128x64 <= 512 ? 15 : (t192 <= 256 && K % 128 == 0) ? 20 : 1;
        return tp;
    }
    tp.variant = (t128 >= 256) ? 1 : 9;
    tp.group_m = 0;
    if (tp.variant == 9) {
        const long t32 = (long)((M + 31) / 32) * ((N + 63) / 64) * par_;
        if (K % 128 == 0 && t32 <= 256) tp.variant = 31;
        else if (K % 128 == 0 && t64 <= 256) tp.variant = 30;
        else if (t64 <= 512) tp.variant = 12;
        else if (epi == vp::EPI_BIAS_RESID_LN && t128x64 <= 512) tp.variant = 15;
        else if (K >= 2048) tp.variant = 12;
    }
    return tp;
}

// Split-K of a residual GEMM at small batches (round 6; in-situ grid profiles/small_batch_r6.txt: 4 models x 1-12 crops x S in {2, 4} x six tiles, whole step timed).
// A call of ONE OR TWO crops leaves most CUs idle in mlp.fc2 -- 72-96 tiles of 32 x 64 per crop, each a serial chain of K / 64 = 48-80 k-blocks: four k ranges per tile
// (288-384 workgroups of 12-20 k-blocks) + the fixed-order reduction kernel win although the partial products make a round trip through L2:
//   1 crop : ViTPose-B 0.575 -> 0.524 ms (-8.9 %), -L 1.376 -> 1.223 (-11.1 %), -H 2.188 -> 1.897 (-13.3 %), -S -1.9 %;   2 crops: -3.9 % / -6.0 % / -4.6 % (B / L / H).
// From 4 crops on the unsplit GEMM fills the chip and the round trip of the partials loses (+1 ... +20 %), with one exception that is shipped: ViTPose-H's mlp.fc2 of
// 7-8 crops (K = 5120 = 80 k-blocks on 480 tiles of 64 x 64) as 4 k ranges of 128 x 128 tiles: 4.435 -> 4.076 ms (-8.1 %).  attn.proj (K = D) never gains.
// Returns S = 1 for everything else; the caller requires K % (128 S) == 0.  A pure function of the shape: tests/test_host_logic.py walks it (vp_dbg_splitk_pick).
SplitKPick pick_splitk(int M, int N, int K) {
    if (K < 3 * N || K % 512 != 0) return {1, 0};         // mlp.fc2 only (K = 4 N)
    if (M <= 192) return {4, N >= 1280 ? 12 : 31};         // one crop: 32 x 64 tiles (64 x 64 on a 4-stage ring for ViTPose-H: measured -13.3 % against -10.5 %)
    if (M <= 384 && K >= 3072) return {4, 12};             // two crops (not ViTPose-S: neutral)
    if (K >= 5120 && M > 1152 && M <= 1536) return {4, 1};  // ViTPose-H, 7-8 crops
    return {1, 0};
}

// (BM, BN, workgroups resident on 256 CUs) of a 2-phase tile configuration the rules above can return: the product rows of tiles.h
static bool tile2_dims(int variant, int& bm, int& bn, int& slots) {
    const vp::TileRow* r = vp::find_tile(variant);
    if (!r || !r->product) return false;
    bm = r->BM; bn = r->BN; slots = vp::tile_slots(*r);
    return true;
}

// Rounds x tile area x K of one MLP GEMM on the tile resolve_gemm picked: the persistent 8-phase kernel runs ceil(tiles / 256) full rounds (its 192-row tile priced x 1.08 as in
// pick_gemm8_tile); a 2-phase launch ceil(tiles / resident slots) rounds, priced x 1.15 (measured: the 2-phase 256 x 256 tile 33 us against 30 for the same one-round launch on
// the 8-phase kernel, the default tile 110 against 80-90).
static double mlp_gemm_cost(const GemmPick& pk, int M, int N, int K) {
    int bm = 192, bn = 128, slots = 512;
    if (const vp::Tile8Row* t8 = vp::find_tile8(pk.variant)) {
        bm = t8->BM; bn = t8->BN;
        return (double)(((long)(M / bm) * (N / bn) + 255) / 256) * bm * bn * (bm == 192 ? 1.08 : 1.0) * K;
    }
    if (!tile2_dims(pk.variant, bm, bn, slots)) return 0.0;
    const long t = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    return (double)((t + slots - 1) / slots) * bm * bn * (slots / 256) * 1.15 * K;
}

// The batch the ENCODER runs for a chunk of n crops (round 6, profiles/small_batch_r6.txt calls 20 + 22): the 8-phase kernel's 256-row tiles need a row count that is a multiple
// of 256 = a multiple of 4 crops, so a batch of 65 crops of ViTPose-L ran mlp.fc2 in 137 us on 516 2-phase tiles where 68 crops take 99 us -- the whole step 9.93 against 9.02 ms.
// From 33 crops on the encoder therefore runs the next multiple of 4 crops (the padding rows repeat the last crop: im2col_launch n_src; every kernel of the path works row by row
// or crop by crop, so the real crops' results are bit for bit those of the unpadded run: test_padded_encoder_batch_is_bit_identical) whenever the cost above of mlp.fc1 + mlp.fc2
// drops by more than 5 % -- checked against the measured step times of every batch size in calls 17-20: 108 of the 112 padded sizes gain (2-9 %), 4 lose 1.0-4.2 %.  The head
// and the decode run the real crops only.  A pure function of (n, D): tests/test_host_logic.py walks it through vp_dbg_run_batch.
static int pick_run_batch(const Switches& s, int n, int D, int limit) {
    const int n4 = (n + 3) / 4 * 4;
    if (n < 33 || n4 == n || n4 > limit) return n;
    auto cost = [&](int m) {
        const int M = 192 * m;
        return mlp_gemm_cost(resolve_gemm(s, VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, M, 4 * D, D), M, 4 * D, D) +
               mlp_gemm_cost(resolve_gemm(s, VP_PROF_GEMM_FC2, vp::EPI_BIAS_RESID_LN, M, D, 4 * D), M, D, 4 * D);
    };
    const double c0 = cost(n), c1 = cost(n4);
    return (c0 > 0.0 && c1 > 0.0 && c1 < 0.95 * c0) ? n4 : n;
}

int tile_bm(int variant) {
    if (const int bm8 = vp::tile8_bm(variant)) return bm8;
    int bm = 0, bn = 0, slots = 0;
    return tile2_dims(variant, bm, bn, slots) ? bm : 0;
}

// ViTPose+ mlp.fc2 of a batch that mixes experts (vp_infer_experts): the host orders the crops by expert, so the experts change only at the crops in `bounds`,
// and a tile reads ONE expert's weights -- it may not span such a change.  Tiles of 32 / 64 / 96 / 192 rows divide a crop (192 token rows) and always qualify;
// 128- and 256-row tiles only where every change falls on a multiple of their height (2 / 4 crops).  The rules above stay as they are: a single-expert batch
// never gets here, and a mixed one keeps the rule's tile wherever it qualifies.  Every fallback is in the one-launch family (same k order, same bits).
bool expert_tile_ok(int bm, const std::vector<int>& bounds) {
    if (bm <= 0) return false;
    for (int b : bounds)
        if (((long)b * 192) % bm) return false;
    return true;
}

// The crop-aligned tile a mixed batch's mlp.fc2 takes where the rule's 128- or 256-row tile spans an expert change: the 8-phase kernel's 192 x 256 tile where the
// 8-phase kernel would have run it (gemm8_ok: N % 256 == 0 and >= 1.75 tiles per CU, ViTPose-B / -L / -H at large batches), else the residual default 192 x 128.
int expert_fallback_variant(int M, int N, bool gemm8_ok, int* group_m) {
    constexpr vp::Tile8Row t8 = *vp::find_tile8(18);   // 192 x 256: the 8-phase tile of one crop's rows
    if (gemm8_ok && N % t8.BN == 0 && (long)(M / t8.BM) * (N / t8.BN) >= 448) { *group_m = 2; return t8.id; }
    *group_m = 0;
    return 11;
}

static int gemm8_group_m(int fam) { return fam == VP_PROF_GEMM_QKV ? 4 : fam == VP_PROF_GEMM_FC2 ? 2 : 8; }   // measured sweep 0 / 2 / 4 / 8 / 16 / 32 (spread 2-3 %)

// The complete choice for one GEMM, in the order the rules override each other: the tuned configuration (tools) or the 2-phase rule; the persistent variant of the
// default wide tile; the 8-phase kernel at large batches; the fused deconv2 + final conv tile; a LayerNorm consumer that folds the statistics itself; a mixed-expert
// batch's crop-aligned fc2 tile; split-K of a residual GEMM of a small batch.
GemmPick resolve_gemm(const Switches& s, int fam, int epi, int M, int N, int K, bool ln_part, size_t splitk_rows, const std::vector<int>* mix_bounds) {
    GemmPick p;
    const bool tuned = s.gemm_variant[fam] >= 0;
    const bool wide = epi == vp::EPI_BIAS || epi == vp::EPI_BIAS_GELU;
    const int w_rows = (int)pad128((size_t)N);
    if (tuned) {
        p.variant = s.gemm_variant[fam]; p.group_m = s.gemm_group_m[fam];
    } else {
        const Tile2Pick tp = pick_gemm2_tile(epi, M, N, K);   // the 2-phase kernels' tile (the 8-phase kernel may take the GEMM over below)
        p.variant = tp.variant; p.group_m = tp.group_m;
    }
    if (s.persist_gemm && p.variant == 8 && wide && K % 128 == 0 && M % 192 == 0 && N % 128 == 0 && (long)(M / 192) * (N / 128) >= 1024)   // >= 2 tiles per resident workgroup
        p.persist = 1;
    // large batches: the 8-phase persistent kernel (gemm8.hip), one 512-thread workgroup per CU on the tile pick_gemm8_tile picks, where the kernel takes the shape
    // (attn.proj, K = N = D, is HBM-bound and stays on the 192 x 128 tile with two workgroups per CU: measured 105 vs 112 us; bit 3 of VP_GEMM8 moves it too)
    const int g8bit = fam == VP_PROF_GEMM_FC2 ? 1 : fam == VP_PROF_GEMM_FC1 ? 2 : fam == VP_PROF_GEMM_QKV ? 4 : fam == VP_PROF_GEMM_PROJ ? 8 : 0;
    if (!tuned && (s.gemm8_mask & g8bit) && (wide || epi == vp::EPI_BIAS_RESID_LN)) {
        const G8Pick pk = pick_gemm8_tile(M, N, wide, s.g8_bm192, s.g8_min_tiles, s.g8_cost_model);
        if (pk.variant && vp::gemm8_shape_ok(epi, M, N, K, N, w_rows, pk.bn, pk.bm)) {
            p.variant = pk.variant; p.group_m = gemm8_group_m(fam); p.persist = 0; p.stagger = s.g8_stagger;
        }
    }
    if (epi == vp::EPI_DECONV_FINAL) { p.variant = 3; p.group_m = 0; p.persist = 0; }   // deconv2 + final 1x1 conv: the 256 x 256 tile (all channels of a pixel)
    if (ln_part) {   // only the one-tile-per-workgroup 2-phase kernel folds partial statistics itself
        p.persist = 0;
        if (is_gemm8(p.variant)) { p.variant = 8; p.group_m = 8; }
    }
    const bool mixed = mix_bounds && fam == VP_PROF_GEMM_FC2;   // ViTPose+ mixed batch: every crop's m-tiles read its own expert's fc2
    if (mixed && !expert_tile_ok(tile_bm(p.variant), *mix_bounds)) {   // a tile would span two experts: the crop-aligned tile instead
        const bool g8 = (s.gemm8_mask & 1) && vp::gemm8_shape_ok(epi, M, N, K, N, w_rows, vp::tile8_bn(18), vp::tile8_bm(18));
        p.variant = expert_fallback_variant(M, N, g8, &p.group_m);
        p.persist = 0;
        p.stagger = p.variant == 18 ? s.g8_stagger : 0;
    }
    // small batches: a residual GEMM as S partial products over k ranges + a fixed-order reduction (pick_splitk); the path's residual GEMMs update x in place
    if (epi == vp::EPI_BIAS_RESID_LN && !mixed && splitk_rows && (size_t)M <= splitk_rows && !tuned && !is_gemm8(p.variant) &&
        (fam == VP_PROF_GEMM_FC2 || fam == VP_PROF_GEMM_PROJ)) {
        const int which = fam == VP_PROF_GEMM_FC2 ? 1 : 0;
        SplitKPick sk = pick_splitk(M, N, K);
        if (s.splitk_force[which][0] > 0) sk = {s.splitk_force[which][0], s.splitk_force[which][1]};
        if (sk.S > 1 && sk.S <= SPLITK_MAX_S && K % (sk.S * 128) == 0) { p.splitk = sk.S; p.splitk_variant = sk.variant; }
    }
    return p;
}

// fp8 mode: tile width 256 for the wide GEMMs; the residual GEMM takes the width whose tile count fills the rounds of 256 persistent workgroups best
GemmPick resolve_gemm_fp8(int fam, int epi, int Mp, int N) {
    int bn = 256;
    if (epi == vp::EPI_BIAS_RESID_LN) {
        double fill = -1.0;
        for (int cand : {256, 192}) {
            if (N % cand) continue;
            const long t = (long)(Mp / 256) * (N / cand);
            if (t < 8) continue;
            const double f = (double)t / (double)up256((size_t)t);
            if (f > fill + 1e-9) { bn = cand; fill = f; }
        }
    }
    GemmPick p;
    p.variant = bn == 192 ? 17 : 16;
    p.group_m = gemm8_group_m(fam);
    return p;
}

// The head of nh crops: large batches run the final 1x1 conv in deconv2's epilogue (gemm.hip EPI_DECONV_FINAL, bit-identical heatmaps) and the [n,64,48,256] tensor is
// never written; small batches keep the two launches on tiles that still fill 256 CUs
HeadPlan plan_head(const Switches& s, int D, int nh, size_t fin_rows, int head_kind) {
    HeadPlan h;
    h.kind = head_kind;
    if (head_kind == 1) return h;   // the simple decoder: one kernel, one shape (simplehead.hip)
    h.fused = s.fuse_head && s.gemm_variant[VP_PROF_GEMM_DECONV] < 0 && (long)nh * 12 >= 512;
    h.deconv1 = resolve_gemm(s, VP_PROF_GEMM_DECONV, vp::EPI_DECONV, nh * 192, 256, 4 * D);
    h.deconv2 = resolve_gemm(s, VP_PROF_GEMM_DECONV, h.fused ? vp::EPI_DECONV_FINAL : vp::EPI_DECONV, nh * 768, 256, 1024);
    if (!h.fused) h.final = resolve_gemm(s, VP_PROF_GEMM_FINAL, vp::EPI_HEATMAP, nh * 3072, (int)fin_rows, 256);
    return h;
}

ChunkPlan plan_chunk(const Switches& s, int D, int heads, int max_batch, bool fp8, int n_in, size_t fin_rows, const std::vector<int>* mix_bounds, int head_kind) {
    ChunkPlan p;
    // the ENCODER's batch: n_in crops, or the next multiple of 4 where that buys the MLP GEMMs an 8-phase tile (pick_run_batch; rows n_in .. n - 1 repeat the last crop and
    // are never read by the head); the fp8 mode pads its rows itself
    p.n = (s.pad_batch && s.fuse_ln && !fp8) ? pick_run_batch(s, n_in, D, (max_batch + 3) / 4 * 4) : n_in;
    const int n = p.n, M = 192 * n, hd = D / heads;
    const size_t splitk_rows = (s.fuse_ln && !fp8 && s.splitk_on) ? (size_t)std::min(max_batch, SPLITK_MAX_CROPS) * 192 : 0;   // vp_create's workspace
    auto gemm = [&](int fam, int epi, int N, int K, bool ln_part) { return resolve_gemm(s, fam, epi, M, N, K, ln_part, splitk_rows, mix_bounds); };
    p.attn_qsplit = (long)n * heads <= s.attn_qsplit;
    p.head = plan_head(s, D, n_in, fin_rows, head_kind);
    const int resid = s.fuse_ln ? vp::EPI_BIAS_RESID_LN : vp::EPI_BIAS_RESID;   // without the fused LayerNorm: standalone passes, fp32 residual stream
    p.gemm[VP_PROF_GEMM_PATCH] = gemm(VP_PROF_GEMM_PATCH, s.fuse_ln ? vp::EPI_POS_LN : vp::EPI_POS, D, 768, false);
    p.gemm[VP_PROF_GEMM_PROJ] = gemm(VP_PROF_GEMM_PROJ, resid, D, D, false);
    if (fp8) {   // qkv / fc1 / fc2 (and attn.proj at head dim 64) on MXFP8 operands, token rows padded to a multiple of 256 (>= 512)
        const int Mp = std::max((int)up256((size_t)M), 512);
        p.proj_fp8 = hd == 64 && !s.fp8_proj16;
        p.gemm[VP_PROF_GEMM_QKV] = resolve_gemm_fp8(VP_PROF_GEMM_QKV, vp::EPI_BIAS, Mp, 3 * D);
        if (p.proj_fp8) p.gemm[VP_PROF_GEMM_PROJ] = resolve_gemm_fp8(VP_PROF_GEMM_PROJ, vp::EPI_BIAS_RESID_LN, Mp, D);
        p.gemm[VP_PROF_GEMM_FC1] = resolve_gemm_fp8(VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, Mp, 4 * D);
        p.gemm[VP_PROF_GEMM_FC2] = resolve_gemm_fp8(VP_PROF_GEMM_FC2, vp::EPI_BIAS_RESID_LN, Mp, D);
        return p;
    }
    p.gemm[VP_PROF_GEMM_FC2] = gemm(VP_PROF_GEMM_FC2, resid, D, 4 * D, false);
    if (!s.fuse_ln) {
        p.gemm[VP_PROF_GEMM_QKV] = gemm(VP_PROF_GEMM_QKV, vp::EPI_BIAS, 3 * D, D, false);
        p.gemm[VP_PROF_GEMM_FC1] = gemm(VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, 4 * D, D, false);
        return p;
    }
    // Small batches: the consumers fold the partial statistics themselves (same code, same bits) -- 2 x depth launches less
    // (round 6: with the consumers' merge on a register copy of the row's statistics instead of a bank-conflicted LDS image -- gemm.hip, GemmArgs::ln_part -- the fold wins at
    // every model and batch up to 8 crops, the one-round 192 x 128 tiles of ViTPose-L included: 8 crops 2.200 -> 2.143 ms against the ln_finalize launches, 4 crops 1.874 ->
    // 1.800, 1 crop 1.172 -> 1.111; beyond 8 crops it still loses (every column tile merges its rows again; ViTPose-H's fused qkv + attention tile needs rowstat):
    // profiles/small_batch_r6.txt call 11)
    const bool fold_stats = n <= s.graph_max_n_stats;
    // Round 6 (profiles/small_batch_r6.txt call 25): beyond 8 crops the fold did not lose because of the merge but because the (mean, rstd) area behind the ring pushes the
    // 80 KiB ring of the default 192 x 128 tile over half the CU's LDS -- ONE workgroup per CU instead of two (+9 ... +12 % per step).  Per consumer (attn.qkv reads LayerNorm-1,
    // mlp.fc1 LayerNorm-2): fold where its GEMM runs on a 2-phase tile that keeps its occupancy with the area (every configuration but the 80 KiB-ring ones), i.e. not on the
    // 8-phase kernel, not in a fused qkv + attention kernel (they read rowstat): ViTPose-S 9-28 crops -6.5 ... -8 %, -B 9-14 -2 ... -6 %, -L 9-10 -2.3 %; same code, same bits.
    auto folds = [&](int fam, int epi, int N) {
        if (fold_stats) return true;
        if (!s.fold_rule || n > 64 || s.gemm_variant[fam] >= 0) return false;
        const int v = gemm(fam, epi, N, D, false).variant;
        return vp::tile_folds_stats(v);
    };
    // attn.qkv + attention core as ONE kernel per (pair of crops, head) from 108 tiles on (qkvattn.hip; bit-identical y; an odd batch's last crop fills both halves of its pair)
    // 128 - 1536 tiles: profiles/qkvattn_r4.txt.  Below (round 6, profiles/small_batch_r6.txt call 16): 108-120 tiles win or tie (ViTPose-B 17-20 crops -0.6 ... -6.5 %: at 19-20
    // crops the unfused qkv is 540 tiles of 128 x 128 on 512 slots; ViTPose-L 13-14 crops equal); 96 tiles and fewer lose (-B 16 crops +-0, 12 crops +3 %, -L 9-12 crops +2 ... +7 %)
    //   Call 26: with the per-consumer statistics fold the two-launch path saves its LayerNorm-1 ln_finalize launches wherever the qkv GEMM's tile folds, and wins back
    //   108-127 tiles there (ViTPose-B 17-18 crops -1.8 / -2.2 %, -L 13-14 crops -2.9 / -3.4 %); where that GEMM would run on the default tile (-B 19-20) the fused kernel keeps them.
    // Head dim 80: one crop x one head per 192 x 256 tile of the 8-phase kernel (gemm8.hip EPI_QKV_ATTN; bit-identical y), from qa80_min_tiles tiles on.
    // The head-major weights both read exist where weights.hip made them (fused LayerNorm, VP_FUSE_QKV_ATTN).
    const bool has_qkvh = s.fuse_qkv_attn && (hd == 64 || (heads * 80 == D && D % 128 == 0));
    const bool qkv_can_fold = folds(VP_PROF_GEMM_QKV, vp::EPI_BIAS, 3 * D);
    const long pair_tiles = (long)((n + 1) / 2) * heads;
    const bool want80 = has_qkvh && heads * 80 == D && (long)n * heads >= s.qa80_min_tiles;
    const bool want64 = has_qkvh && heads * 64 == D && pair_tiles >= s.qa_min_tiles && (s.qa_min_set || pair_tiles >= 128 || !qkv_can_fold);
    p.fold1 = fold_stats || (!want80 && !want64 && qkv_can_fold);   // LayerNorm-1 -> attn.qkv
    p.fold2 = folds(VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, 4 * D);     // LayerNorm-2 -> mlp.fc1
    // (a shape the fused kernels reject -- a chunk beyond their 32-bit row offsets, fewer than 8 tiles under a lowered threshold -- takes the gemm + attention pair)
    vp::QkvAttnArgs qa{};
    qa.npairs = (n + 1) / 2; qa.ncrops = n; qa.heads = heads; qa.D = D;
    if (s.gemm_variant[VP_PROF_GEMM_QKV] < 0 && !p.fold1) {
        if (want80 && vp::gemm8_shape_ok(vp::EPI_QKV_ATTN, M, heads * 256, D, D, heads * 256, 256, 192)) p.qkv_path = QKV_ATTN80;
        else if (want64 && vp::qkvattn_supported(qa)) p.qkv_path = QKV_ATTN64;
    }
    p.gemm[VP_PROF_GEMM_QKV] = gemm(VP_PROF_GEMM_QKV, vp::EPI_BIAS, 3 * D, D, p.fold1);
    p.gemm[VP_PROF_GEMM_FC1] = gemm(VP_PROF_GEMM_FC1, vp::EPI_BIAS_GELU, 4 * D, D, p.fold2);
    return p;
}

}  // namespace vpi

extern "C" {

// HOST ONLY: the tile mlp.fc2 of a mixed-expert batch runs (n crops, the experts change at the n_bounds crops in bounds, embed dim D): `variant` = what the rules picked
// for the row count, gemm8_ok = the 8-phase kernel may run it; returns the variant kept or the crop-aligned fallback
VP_API int vp_dbg_expert_tile(int32_t variant, int32_t M, int32_t N, int32_t gemm8_ok, const int32_t* bounds, int32_t n_bounds) {
    if (M <= 0 || N <= 0 || n_bounds < 0 || (n_bounds > 0 && !bounds)) return VP_ERR_INVALID;
    const std::vector<int> b(bounds, bounds + n_bounds);
    if (expert_tile_ok(tile_bm(variant), b)) return variant;
    int gm = 0;
    return expert_fallback_variant(M, N, gemm8_ok != 0, &gm);
}

// HOST ONLY: the batch the encoder runs for a chunk of n crops of a model of embed dim D (pick_run_batch with the default switches; limit = the handle's padded workspace batch)
VP_API int vp_dbg_run_batch(int32_t n, int32_t D, int32_t limit) {
    if (n <= 0 || D <= 0) return VP_ERR_INVALID;
    return pick_run_batch(Switches{}, n, D, limit);
}

// HOST ONLY: the plan of a chunk of n crops on a handle of *cfg, with the switches vp_create would read from the environment now; layout: include/vitpose_hip.h
VP_API int vp_dbg_chunk_plan(const vp_config* cfg, int32_t n, int32_t* out, int32_t cap) {
    if (!cfg || cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->embed_dim % cfg->num_heads || cfg->num_keypoints <= 0 || cfg->max_batch <= 0 ||
        n <= 0 || n > cfg->max_batch || cap < 0 || (cap > 0 && !out))
        return VP_ERR_INVALID;
    Switches s;
    read_switches(s);
    const ChunkPlan p = plan_chunk(s, cfg->embed_dim, cfg->num_heads, cfg->max_batch, cfg->dtype == VP_DTYPE_FP8, n, final_rows((size_t)cfg->num_keypoints));
    std::vector<int32_t> v = {p.n, p.fold1, p.fold2, p.qkv_path, p.attn_qsplit, p.head.fused, p.proj_fp8};
    for (const GemmPick& g : {p.gemm[VP_PROF_GEMM_PATCH], p.gemm[VP_PROF_GEMM_QKV], p.gemm[VP_PROF_GEMM_PROJ], p.gemm[VP_PROF_GEMM_FC1], p.gemm[VP_PROF_GEMM_FC2],
                              p.head.deconv1, p.head.deconv2, p.head.final})
        v.insert(v.end(), {g.variant, g.group_m, g.persist, g.stagger, g.splitk, g.splitk_variant});
    std::copy(v.begin(), v.begin() + std::min<size_t>(v.size(), (size_t)cap), out);
    return (int)v.size();
}


// HOST ONLY: the 8-phase tile the selection rule of gemm() picks for an [M, N] output (wide: qkv / fc1; else the residual GEMMs); returns the
// variant (0 = none: 2-phase kernels, 16 = 256 x 256, 17 = 256 x 192, 18 = 192 x 256) and its tile count
VP_API int vp_dbg_gemm8_pick(int32_t M, int32_t N, int32_t wide, int32_t bm192_mask, int32_t* tiles) {
    if (M <= 0 || N <= 0) return VP_ERR_INVALID;
    const G8Pick pk = pick_gemm8_tile(M, N, wide != 0, bm192_mask & 3, 448, !(bm192_mask & 4));
    if (tiles) *tiles = (int32_t)pk.tiles;
    return pk.variant;
}

// HOST ONLY: the tile configuration (gemm.hip Cfg id) the 2-phase selection rule picks for one GEMM: epi = kernels.h GemmEpi (0 bias, 1 bias + GELU, 4 deconv, 5 heatmap,
// 6 residual + statistics, 7 pos + statistics), shape [M, N] x K; *group_m = its tile-order group
VP_API int vp_dbg_gemm2_pick(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t* group_m) {
    if (M <= 0 || N <= 0 || K <= 0) return VP_ERR_INVALID;
    const Tile2Pick tp = pick_gemm2_tile(epi, M, N, K);
    if (group_m) *group_m = tp.group_m;
    return tp.variant;
}

// HOST ONLY: the split-K rule for a residual GEMM of [M, N] x K: returns S (1 = one launch), *variant = the tile configuration of the partial products
VP_API int vp_dbg_splitk_pick(int32_t M, int32_t N, int32_t K, int32_t* variant) {
    if (M <= 0 || N <= 0 || K <= 0) return VP_ERR_INVALID;
    const SplitKPick sk = pick_splitk(M, N, K);
    if (variant) *variant = sk.variant;
    return sk.S;
}

}  // extern "C"
