// vrg_rim.h - the arithmetic of the rim groups' count (dense pass, option dense_memo = 2; rim_groups in vrg_device.hip), kept apart
// from the wave's cross-lane steps so that a host program can run it: tests/test_dense_rim_memo.py compiles this header alone and
// compares it with plain population counts.  Nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VRG_RIM_HD __host__ __device__ inline
#else
#define VRG_RIM_HD inline
#endif

// A lane's class word holds four groups of four voxels, two bits per voxel (bit 1 of a pair: outer).  Returns the lane's outer voxels
// of each group, one count (0..4) per byte.  The wave adds these words with plain 32-bit additions: over 32 lanes a byte reaches at
// most 128 and never carries into the next.
VRG_RIM_HD uint32_t vrg_rim_pack(uint32_t w) {
    uint32_t x = (w >> 1) & 0x55555555u;
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0f0f0f0fu;
}
// a, b: the 32-bit sums of the packed words of lanes 0..31 and 32..63 (each byte <= 128; their sum, up to 256, is formed here in 32
// bits); inner: the groups in which a lane holds an inner voxel; ic01, ic23: the four counts of init, 16 bits each.  Returns the groups
// that take their sum from the table: no inner voxel, as many outer voxels as init counted included ones, not 0.  ne: the groups that
// hold an included voxel; nouter: the unit's outer voxels.
VRG_RIM_HD uint32_t vrg_rim_decide(uint32_t a, uint32_t b, uint32_t inner, uint32_t ic01, uint32_t ic23, uint32_t& ne, uint32_t& nouter) {
    uint32_t m = 0u, some = 0u;
    nouter = 0u;
    for (int j = 0; j < 4; j++) {
        const uint32_t n = ((a >> (8 * j)) & 0xffu) + ((b >> (8 * j)) & 0xffu);
        const uint32_t ic = ((j < 2 ? ic01 : ic23) >> (16 * (j & 1))) & 0xffffu;
        if (n == ic && n != 0u) m |= 1u << j;
        if (n != 0u) some |= 1u << j;
        nouter += n;
    }
    ne = some | inner;
    return m & ~inner;
}

// ---- the unit-level decision of the walk's short way (k_recount_bits, RIM) ------------------------------------------------------
// A trip of the walk takes the short way - every group's sum from the table, no intensity load - iff every group of its units that
// holds an included voxel passes vrg_rim_decide.  That needs no count per group.  Inclusion is monotone: a voxel never becomes
// excluded, and the excluded bit is set by init alone, so the included set of a group only grows.  In a unit without inner voxels
// the outer voxels are the included ones, hence group by group a superset of init's included set: n_j >= icnt_j for all four groups.
// Equal TOTALS, sum n_j == sum icnt_j, then force n_j == icnt_j in every group - each non-empty group matches its count, and a group
// with n_j == 0 is empty and was empty at init (its table sum is +0.0).  Conversely a unit whose groups all pass has no inner voxel
// and equal totals.  So: one population count per lane and unit (<= 16), one sum over the wave per unit (<= 1024), one comparison.
//
// Two units share a 32-bit word as 16-bit fields: a field reaches at most 1024 over the 64 lanes and never carries into the other.
// A trip holds three units; the fourth field counts the INNER voxels of all three (the inner bits of the OR of the three words: a word
// has 16 of them, so at most 16 per lane and 1024 over the wave; 0 iff no lane holds an inner voxel in any of the three), against an
// expected count of 0, which folds "no lane holds an inner voxel" into the same sums.
// The counts of init enter the same sums with a minus sign: the unit's four counts are two words of two 16-bit counts, each word
// fetched by ONE lane (lanes 4 q and 4 q + 1 for slot q of the trip), which subtracts the sum of its two counts (vrg_unit_share,
// at most 512) from the unit's field of its own word (vrg_unit_role01 / vrg_unit_role2i: -1, -65536 or 0 by the lane).  The wave adds
// the words of its lanes with plain 32-bit additions (six DPP steps; any order gives the same totals, the arithmetic is modulo 2^32),
// and the total of a word is D_lo + 65536 D_hi (mod 2^32) with D = a field's outer (inner) voxels minus what init counted,
// |D| <= 1024: it is 0 iff D_lo = D_hi = 0, for |D_lo + 65536 D_hi| < 2^32 makes it 0 as an integer, 65536 then divides D_lo, so
// D_lo = 0 and with it D_hi.  The trip takes the short way iff both totals are 0 (vrg_unit_short).
VRG_RIM_HD uint32_t vrg_unit_outer(uint32_t w) { return (uint32_t)__builtin_popcount(w & 0xAAAAAAAAu); }
// units 0 and 1 of a trip: this lane's outer voxels of each, one per field
VRG_RIM_HD uint32_t vrg_unit_pack01(uint32_t w0, uint32_t w1) { return vrg_unit_outer(w0) | (vrg_unit_outer(w1) << 16); }
// unit 2 and the inner voxels of all three
VRG_RIM_HD uint32_t vrg_unit_pack2i(uint32_t w0, uint32_t w1, uint32_t w2) {
    return vrg_unit_outer(w2) | ((uint32_t)__builtin_popcount((w0 | w1 | w2) & 0x55555555u) << 16);
}
// d: one word of a unit's counts of init (two counts of at most 256) -> their sum
VRG_RIM_HD uint32_t vrg_unit_share(uint32_t d) { return (d & 0xffffu) + (d >> 16); }
// what lane `lane` multiplies its share by before adding it to its two words: lanes 0, 1 hold the counts of slot 0, lanes 4, 5 those of
// slot 1, lanes 8, 9 those of slot 2; every other lane's share counts for nothing
VRG_RIM_HD int32_t vrg_unit_role01(uint32_t lane) { return lane < 2u ? -1 : ((lane & ~1u) == 4u ? -65536 : 0); }
VRG_RIM_HD int32_t vrg_unit_role2i(uint32_t lane) { return (lane & ~1u) == 8u ? -1 : 0; }
VRG_RIM_HD uint32_t vrg_unit_mul(uint32_t share, int32_t role) {
    const int32_t r24 = (int32_t)((uint32_t)role << 8) >> 8;               // (the role as it is, visibly 24 bits wide: one full-rate multiply-add on the device)
    return (uint32_t)((int32_t)(share & 0x3ffu) * r24);
}
// a lane's two words of a trip: packed counts minus its share of init's
VRG_RIM_HD uint32_t vrg_unit_word01(uint32_t w0, uint32_t w1, uint32_t share, int32_t role01) { return vrg_unit_pack01(w0, w1) + vrg_unit_mul(share, role01); }
VRG_RIM_HD uint32_t vrg_unit_word2i(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t share, int32_t role2i) { return vrg_unit_pack2i(w0, w1, w2) + vrg_unit_mul(share, role2i); }
// t01, t2i: the sums of the two words over the wave's 64 lanes
VRG_RIM_HD bool vrg_unit_short(uint32_t t01, uint32_t t2i) { return (t01 | t2i) == 0u; }

// ---- one count per TURN of the short way (k_recount_bits, RIM: a turn is RIM_TRIPS trips) ------------------------------------------
// The argument above does not stop at a trip: ONE word decides a turn of any number of units.  A lane's word holds two fields.  The
// low one is the lane's outer voxels of ALL units of the turn, minus its share of init's counts: lanes 4 q and 4 q + 1 (q < 3) of
// every trip hold that trip's count words exactly as vrg_unit_share reads them, so such a lane subtracts the sum of its shares over
// the turn's trips (vrg_turn_mask: all ones in those six lanes, 0 elsewhere).  The high field (<< 16) is the population count of the
// inner bits of the OR of all the turn's class words.  The wave adds the words with plain 32-bit additions and looks at the total:
//   I, the total's inner field, is 0 iff no lane holds an inner voxel in any unit of the turn.  Then, by monotone inclusion, every
//     unit has at least as many outer voxels as init counted included ones: D = sum over the units of (outer - icnt) is a sum of
//     terms >= 0 and is 0 iff every unit matches its count - the per-unit condition above, for every unit of every trip.
//   If I > 0 some trip holds an inner voxel and the turn must fail whatever D is: a unit with inner voxels can hold FEWER outer voxels
//     than init counted, and its deficit may cancel another unit's surplus - which is why the inner count has a field of its own and
//     cannot be added into D's.
//   Widths: a lane's OR has 16 inner bits, so I <= 1024 over the wave; |D| <= 1024 per unit, so |D| < 65536 with at most 63 units
//     per turn (VRG_TURN_MAX_UNITS).  The total is D + 65536 I (mod 2^32) with 0 <= 65536 I <= 2^26: if I = 0 it is D mod 2^32, 0 iff
//     D = 0; if I >= 1 it lies in (0, 2^26 + 2^16) as an integer and is not 0.  So the total is 0 iff D = I = 0.
// A turn passes iff every one of its trips passes vrg_unit_short (tests/test_dense_turn.py runs both on the host).
constexpr int VRG_TURN_MAX_UNITS = 63;
VRG_RIM_HD uint32_t vrg_turn_mask(uint32_t lane) { return (lane < 12u && (lane & 2u) == 0u) ? 0xffffffffu : 0u; }
// outer: the lane's outer voxels of all the turn's units (the sum of vrg_unit_outer); orw: the OR of their class words; shares: the sum
// of vrg_unit_share over the lane's count words of the turn's trips
VRG_RIM_HD uint32_t vrg_turn_word(uint32_t outer, uint32_t orw, uint32_t shares, uint32_t mask) {
    return outer - (shares & mask) + ((uint32_t)__builtin_popcount(orw & 0x55555555u) << 16);
}
// total: the sum of the words over the wave's 64 lanes
VRG_RIM_HD bool vrg_turn_short(uint32_t total) { return total == 0u; }
