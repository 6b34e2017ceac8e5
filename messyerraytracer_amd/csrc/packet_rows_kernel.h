// packet_rows_kernel.h — the packet walk written end to end in gfx950 assembly: 64 rays (one packet) or 128 rays
// (two 8x8 tiles sharing ONE walk) per wave.  Included by kernels.hip (inside namespace mrt, after packet_asm_kernel.h).
//
// What round 2 measured about trace_packet_asm_kernel (profiles/r02a_*, r02b_*):
//   * occupancy sweep (tools/exp_occupancy.py): 8 / 4 / 2 waves per SIMD run C3 in 2.29 / 4.46 / 8.77 ms: a wave's
//     lifetime does not depend on how many others are resident; the vector ALUs sit at 0.55 of their issue rate;
//   * s_memtime clock (tools/exp_walk_clock.py): a row fetch costs ~200 cycles and these waits are 30-40 % of a
//     wave's life at C3 (45 % at C5); the rest is the wave's own instruction stream at ~12 cycles per instruction;
//   * the triangle loads of the leaf code were never scalar (SQ_INSTS_VMEM_RD 91 per wave): three vector loads per
//     triangle, behind an s_waitcnt vmcnt(0) that also waited for the far-child prefetches;
//   * two packets per wave walked SEPARATELY in lockstep (one wait for two fetches) halved the waits and nothing
//     else: 2.19 against 2.15 ms.  Retired.
// So the lever is the instruction stream and the fetches PER RAY.  This kernel
//   * keeps the whole walk inside one assembly block: ONE row array holds the scene's wide nodes followed by its
//     triangles as 64-byte rows ({v0,id | e1,layers | e2,flags | normal}, the reference's GPUTrianglePacked row),
//     leaf refs rebased to row indices, so a packet's current item — inner node or triangle — is always
//     `rows[ref & 0x3FFFFFF]`: one s_load_dwordx16 through the scalar cache, address = one shift; the triangle test
//     (Moller-Trumbore, the correctly rounded 1/det sequence, the tie rule, per-lane ownership) is in the block too;
//   * and gives a wave TWO rays per lane (groups A and B = two neighbouring 8x8 tiles) that share one walk: one
//     fetch, one stack, one near/far decision per step for 128 rays, the slab / triangle arithmetic once per group
//     — and only for a group that has a lane owning the row (ownership masks per group travel with every stack
//     entry), so a group never tests a row its own 64-ray walk would not have reached.  Scalar work, branches,
//     stack traffic and fetch waits per ray drop by the share of rows the two tiles have in common (most of them
//     when a tile is smaller than a triangle).
//
// Arithmetic is the canonical form of DESIGN.md (the same fma / mul sequences the compiler emits for
// packet_leaf and the lane kernels: explicit fma, nothing contracted, 1/det correctly rounded by the
// v_div_scale / v_rcp / v_div_fmas / v_div_fixup sequence), so results stay bit-identical to the oracle.
// gfx950 hazards respected by construction: a lane mask written by v_cmp is consumed by the scalar ALU, or by a
// vector instruction at least two instructions later; v_rcp's result is first read two instructions later;
// v_div_scale's VCC reaches v_div_fmas six instructions later.
#pragma once

// ---- fixed registers ----------------------------------------------------------------------------------------
// the current row: s[20:35]
//   node row:     lmin.xyz lref | lmax.xyz rref | rmin.xyz - | rmax.xyz -
//   triangle row: v0.xyz id | e1.xyz layers | e2.xyz flags | normal (unused here)
// own masks (the lanes whose own ray hit the current row's box): group A s[60:61], group B s[62:63]
// scratch: s52 (byte offset; the counting builds' copy of sp), s53 (far ref); lane-mask pairs of the triangle test s[54:55]
// (accepting lanes), s[56:57], s[58:59], s[64:65], s[66:67]; of the 128-ray node step s[36:37] / s[38:39] (group A hit left /
// right), s[40:41] / s[42:43] (group B), s[44:45] (any lane hit left; the culling loop's cull word), s[46:47] (left-is-nearer
// flags), s48 / s49 (byte offsets of the child prefetches; s48 the cull bits of one child), s[50:51] / s[58:59] (the pushed
// child's masks).  s64 / s65 are also the never-read destinations of the 128-ray walk's child prefetches, s[64:67] the counting
// builds' clock, s[66:67] in the culling loop "the current row's copy is the one in v61".  s68: the stack's top, in
// MRT_ROWS_POPFETCH builds only (the kernel has 72 scalars below the compiler's).  s[70:71]: the EXEC the paired walk's general code was
// entered with, in MRT_ROWS_OWNEXEC builds only.
// v50..v59 temporaries; v60 the never-read destination of the one-packet loop's far-child prefetch, a product of the packed node
// step (MRT_ROWS_PKSLAB), in the culling loop the vector copy of the left child's (or the popped) row; v61 the right child's
// copy and v62 the address of a copy's request, both in the culling loop only.
// The four-wide loop (packet_quad_kernel.h) reads a 128-byte row into s[20:51] and keeps its own masks in s[68:71]: its register
// comment is in that file.
#define RA_LMINX "s20"
#define RA_LMINY "s21"
#define RA_LMINZ "s22"
#define RA_LREF "s23"
#define RA_LMAXX "s24"
#define RA_LMAXY "s25"
#define RA_LMAXZ "s26"
#define RA_RREF "s27"
#define RA_RMINX "s28"
#define RA_RMINY "s29"
#define RA_RMINZ "s30"
#define RA_RMAXX "s32"
#define RA_RMAXY "s33"
#define RA_RMAXZ "s34"
#define RA_MASK "s[60:61]"
#define RA_MASKLO "s60"
#define RA_MASKHI "s61"
// the same registers read as a triangle row
#define RA_V0X "s20"
#define RA_V0Y "s21"
#define RA_V0Z "s22"
#define RA_ID "s23"
#define RA_E1X "s24"
#define RA_E1Y "s25"
#define RA_E1Z "s26"
#define RA_LAYERS "s27"
#define RA_E2X "s28"
#define RA_E2Y "s29"
#define RA_E2Z "s30"
#define RA_FLAGS "s31"

// near / far plane of an axis by the sign bit of the octant (0: inv >= 0 -> near = min, far = max; 1: swapped)
#define MRT_NEAR_0(RS, AX, SIDE) RS##_##SIDE##MIN##AX
#define MRT_NEAR_1(RS, AX, SIDE) RS##_##SIDE##MAX##AX
#define MRT_FAR_0(RS, AX, SIDE) RS##_##SIDE##MAX##AX
#define MRT_FAR_1(RS, AX, SIDE) RS##_##SIDE##MIN##AX

// operand of packet P ("A" / "B"): %[oxA] ...
#define MRT_OP(NAME, P) "%[" NAME P "]"

// slab test of one 64-ray group against both child boxes of the node row (ray_aabb, glsl:84-99, octant-specialised:
// near / far plane of each axis known from the sign of the direction).  v50 = tl, v53 = tlx (entry / exit of the left
// box clamped to [t_min, lim]), v56 = tr, v52 = trx.  Ordered so that no instruction reads its predecessor's result.
#define MRT_ROWS_SLAB(P, RS, BX, BY, BZ)                                                                             \
	"v_fma_f32 v50, " MRT_NEAR_##BX(RS, X, L) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                        \
	"v_fma_f32 v51, " MRT_NEAR_##BY(RS, Y, L) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                        \
	"v_fma_f32 v52, " MRT_NEAR_##BZ(RS, Z, L) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                        \
	"v_fma_f32 v53, " MRT_FAR_##BX(RS, X, L) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                         \
	"v_fma_f32 v54, " MRT_FAR_##BY(RS, Y, L) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                         \
	"v_fma_f32 v55, " MRT_FAR_##BZ(RS, Z, L) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                         \
	"v_max_f32 v52, v52, " MRT_OP("tmin", P) "\n"                                                                   \
	"v_fma_f32 v56, " MRT_NEAR_##BX(RS, X, R) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                        \
	"v_min_f32 v55, v55, " MRT_OP("lim", P) "\n"                                                                    \
	"v_fma_f32 v57, " MRT_NEAR_##BY(RS, Y, R) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                        \
	"v_max3_f32 v50, v50, v51, v52\n"        /* v50 = tl  */                                                       \
	"v_fma_f32 v51, " MRT_NEAR_##BZ(RS, Z, R) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                        \
	"v_min3_f32 v53, v53, v54, v55\n"        /* v53 = tlx */                                                       \
	"v_fma_f32 v52, " MRT_FAR_##BX(RS, X, R) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                         \
	"v_fma_f32 v54, " MRT_FAR_##BY(RS, Y, R) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                         \
	"v_fma_f32 v55, " MRT_FAR_##BZ(RS, Z, R) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                         \
	"v_max_f32 v51, v51, " MRT_OP("tmin", P) "\n"                                                                   \
	"v_min_f32 v55, v55, " MRT_OP("lim", P) "\n"                                                                    \
	"v_max3_f32 v56, v56, v57, v51\n"        /* v56 = tr  */                                                       \
	"v_min3_f32 v52, v52, v54, v55\n"        /* v52 = trx */

// ---- one node step of a 64-ray packet (register set RS, octant bits BX BY BZ) -------------------------------------
// Ends with cur = the child to visit next (an inner node, or a leaf = its first triangle row, bit 31 set) and the
// mask of the lanes whose own ray hit that child in the packet's mask register; or with the packet's pop bit set
// in %[ev].  A pushed entry is 16 bytes {ref, -, lane mask}.
#define MRT_ROWS_NODE_STEP(P, RS, POPBIT, CNT_P, BX, BY, BZ)                                                                 \
	MRT_ROWS_SLAB(P, RS, BX, BY, BZ)                                                                                \
	"v_cmp_le_f32 vcc, v50, v53\n"           /* lanes that hit the left child  */                                  \
	"v_cmp_le_f32_e64 s[54:55], v56, v52\n"  /* lanes that hit the right child */                                  \
	"s_cbranch_vccz L_" P "lmiss_%=\n"                                                                              \
	"s_cmp_eq_u64 s[54:55], 0\n"                                                                                    \
	"s_cbranch_scc1 L_" P "onlyl_%=\n"                                                                              \
	"v_cmp_lt_f32_e64 s[56:57], v50, v56\n"  /* both hit: lane 0 decides which is nearer (order = speed only) */   \
	"s_bitcmp1_b32 s56, 0\n"                                                                                        \
	"s_cselect_b32 s53, " RS##_RREF ", " RS##_LREF "\n"                  /* far  */                                  \
	"s_cselect_b32 " MRT_OP("cur", P) ", " RS##_LREF ", " RS##_RREF "\n" /* near */                                  \
	"s_cselect_b64 s[58:59], s[54:55], vcc\n"        /* lanes that hit the far child  */                           \
	MRT_ROWS_TOP_PUSHED \
	"s_cselect_b64 " RS##_MASK ", vcc, s[54:55]\n"    /* lanes that hit the near child */                           \
	"v_mov_b32 v51, s53\n"                                                                                          \
	"v_mov_b32 v52, s58\n"                                                                                          \
	"v_mov_b32 v53, s59\n"                                                                                          \
	"ds_write_b32 " MRT_OP("sp", P) ", v51\n"                                                                       \
	"ds_write_b64 " MRT_OP("sp", P) ", v[52:53] offset:8\n"                                                         \
	"v_add_u32 " MRT_OP("sp", P) ", 16, " MRT_OP("sp", P) "\n"                                                      \
	CNT_P                                                                                                           \
	"v_lshlrev_b32 v54, 6, v51\n"            /* pull the pushed row (node, or the leaf's first triangle) towards */ \
	"global_load_dword v60, v54, %[rows]\n"  /* the L2 now; v60 is never read (vmcnt drained at the very end)    */ \
	"s_branch L_" P "done_%=\n"                                                                                     \
	"L_" P "onlyl_%=:\n"                                                                                            \
	"s_mov_b32 " MRT_OP("cur", P) ", " RS##_LREF "\n"                                                                \
	"s_mov_b64 " RS##_MASK ", vcc\n"                                                                                 \
	"s_branch L_" P "done_%=\n"                                                                                     \
	"L_" P "lmiss_%=:\n"                                                                                            \
	"s_cmp_eq_u64 s[54:55], 0\n"                                                                                    \
	"s_cbranch_scc1 L_" P "npop_%=\n"                                                                               \
	"s_mov_b32 " MRT_OP("cur", P) ", " RS##_RREF "\n"                                                                \
	"s_mov_b64 " RS##_MASK ", s[54:55]\n"                                                                            \
	"s_branch L_" P "done_%=\n"                                                                                     \
	"L_" P "npop_%=:\n"                                                                                             \
	"s_or_b32 %[ev], %[ev], " POPBIT "\n"

// ---- one triangle step of packet P: ray_triangle, glsl:105-131 == Triangle::intersect, src/core/triangle.h:56-105,
// in the operation order of packet_leaf() (packet_asm_kernel.h).  The lanes that own the leaf (the packet's mask
// register) test against lim (best_t, or -FLT_MAX for a lane that takes no part); an exact tie goes to the lower id.
// P: the group (operand names, labels); RS: the row's registers; OWNMASK: the lanes of the group that own the leaf;
// CUROP: the operand holding the row ref.  ANYHIT_CODE: what an accepting lane's limit becomes (MRT_ROWS_NEAREST /
// MRT_ROWS_ANYHIT / MRT_ROWSW_ANYHIT).  Falls out at label L_<P>tnext.
#define MRT_ROWS_TRI_TEST(P, RS, OWNMASK, CUROP, ANYHIT_CODE)                                                        \
	"s_and_b32 s52, " RS##_LAYERS ", %[qmask]\n"  /* Triangle layers & query mask (wave-uniform) */                  \
	"s_cbranch_scc0 L_" P "tnext_%=\n"                                                                              \
	"v_mul_f32 v50, " RS##_E2Y ", " MRT_OP("dz", P) "\n"                                                             \
	"v_mul_f32 v51, " RS##_E2Z ", " MRT_OP("dx", P) "\n"                                                             \
	"v_mul_f32 v52, " RS##_E2X ", " MRT_OP("dy", P) "\n"                                                             \
	"v_fma_f32 v50, " MRT_OP("dy", P) ", " RS##_E2Z ", -v50\n"   /* pvx = dy e2z - dz e2y */                         \
	"v_fma_f32 v51, " MRT_OP("dz", P) ", " RS##_E2X ", -v51\n"   /* pvy = dz e2x - dx e2z */                         \
	"v_fma_f32 v52, " MRT_OP("dx", P) ", " RS##_E2Y ", -v52\n"   /* pvz = dx e2y - dy e2x */                         \
	"v_mul_f32 v53, " RS##_E1Z ", v52\n"                                                                             \
	"v_fma_f32 v53, " RS##_E1Y ", v51, v53\n"                                                                        \
	"v_fma_f32 v53, " RS##_E1X ", v50, v53\n"                    /* det = e1 . pv */                                 \
	"v_cmp_nlt_f32_e64 s[54:55], |v53|, %[eps]\n"               /* !(|det| < 1e-8) */                               \
	"s_and_b64 s[54:55], s[54:55], " OWNMASK "\n"               /* ... among the lanes that own this leaf */        \
	"s_cbranch_scc0 L_" P "tnext_%=\n"                                                                              \
	"v_div_scale_f32 v54, s[56:57], v53, v53, 1.0\n"            /* inv_det = 1.0f / det, correctly rounded */       \
	"v_rcp_f32 v55, v54\n"                                                                                          \
	"v_div_scale_f32 v56, vcc, 1.0, v53, 1.0\n"                                                                     \
	"v_subrev_f32 v59, " RS##_V0X ", " MRT_OP("ox", P) "\n"      /* tvx = ox - v0x (also keeps v_rcp's result apart from its first use) */ \
	"v_fma_f32 v57, -v54, v55, 1.0\n"                                                                               \
	"v_fma_f32 v55, v57, v55, v55\n"                                                                                \
	"v_mul_f32 v57, v56, v55\n"                                                                                     \
	"v_fma_f32 v58, -v54, v57, v56\n"                                                                               \
	"v_fma_f32 v57, v58, v55, v57\n"                                                                                \
	"v_fma_f32 v54, -v54, v57, v56\n"                                                                               \
	"v_div_fmas_f32 v54, v54, v55, v57\n"                                                                           \
	"v_div_fixup_f32 v54, v54, v53, 1.0\n"                      /* v54 = inv_det */                                 \
	"v_subrev_f32 v55, " RS##_V0Y ", " MRT_OP("oy", P) "\n"      /* tvy */                                           \
	"v_subrev_f32 v56, " RS##_V0Z ", " MRT_OP("oz", P) "\n"      /* tvz */                                           \
	"v_mul_f32 v58, v56, v52\n"                                                                                     \
	"v_fma_f32 v58, v55, v51, v58\n"                                                                                \
	"v_fma_f32 v58, v59, v50, v58\n"                                                                                \
	"v_mul_f32 v58, v58, v54\n"                                 /* v58 = u = (tv . pv) inv_det */                   \
	"v_cmp_nlt_f32_e64 s[56:57], v58, 0\n"                      /* !(u < 0) */                                      \
	"v_cmp_ngt_f32_e64 s[58:59], v58, 1.0\n"                    /* !(u > 1) */                                      \
	"s_and_b64 s[54:55], s[54:55], s[56:57]\n"                                                                      \
	"s_and_b64 s[54:55], s[54:55], s[58:59]\n"                                                                      \
	"s_cbranch_scc0 L_" P "tnext_%=\n"                                                                              \
	"v_mul_f32 v50, " RS##_E1Y ", v56\n"                                                                             \
	"v_mul_f32 v51, " RS##_E1Z ", v59\n"                                                                             \
	"v_mul_f32 v52, " RS##_E1X ", v55\n"                                                                             \
	"v_fma_f32 v50, v55, " RS##_E1Z ", -v50\n"                   /* qvx = tvy e1z - tvz e1y */                       \
	"v_fma_f32 v51, v56, " RS##_E1X ", -v51\n"                   /* qvy = tvz e1x - tvx e1z */                       \
	"v_fma_f32 v52, v59, " RS##_E1Y ", -v52\n"                   /* qvz = tvx e1y - tvy e1x */                       \
	"v_mul_f32 v59, " MRT_OP("dz", P) ", v52\n"                                                                     \
	"v_fma_f32 v59, " MRT_OP("dy", P) ", v51, v59\n"                                                                \
	"v_fma_f32 v59, " MRT_OP("dx", P) ", v50, v59\n"                                                                \
	"v_mul_f32 v59, v59, v54\n"                                 /* v59 = v = (d . qv) inv_det */                    \
	"v_add_f32 v55, v58, v59\n"                                 /* u + v */                                         \
	"v_cmp_nlt_f32_e64 s[56:57], v59, 0\n"                      /* !(v < 0) */                                      \
	"v_cmp_ngt_f32_e64 s[58:59], v55, 1.0\n"                    /* !(u + v > 1) */                                  \
	"s_and_b64 s[54:55], s[54:55], s[56:57]\n"                                                                      \
	"s_and_b64 s[54:55], s[54:55], s[58:59]\n"                                                                      \
	"s_cbranch_scc0 L_" P "tnext_%=\n"                                                                              \
	"v_mul_f32 v55, " RS##_E2Z ", v52\n"                                                                             \
	"v_fma_f32 v55, " RS##_E2Y ", v51, v55\n"                                                                        \
	"v_fma_f32 v55, " RS##_E2X ", v50, v55\n"                                                                        \
	"v_mul_f32 v55, v55, v54\n"                                 /* v55 = t = (e2 . qv) inv_det */                   \
	/* accept: !(t < t_min) && (t < lim || (t == lim && a hit is held && id < its id)) */                          \
	"v_cmp_nlt_f32_e64 s[56:57], v55, " MRT_OP("tmin", P) "\n"                                                      \
	"v_cmp_lt_f32_e64 s[58:59], v55, " MRT_OP("lim", P) "\n"                                                        \
	"v_cmp_eq_f32_e64 s[64:65], v55, " MRT_OP("lim", P) "\n"                                                        \
	"v_cmp_ne_u32_e64 s[66:67], " MRT_OP("bs", P) ", -1\n"                                                          \
	"v_cmp_gt_u32_e64 vcc, " MRT_OP("bi", P) ", " RS##_ID "\n"   /* id < best_id */                                  \
	"s_and_b64 s[64:65], s[64:65], s[66:67]\n"                                                                      \
	"s_and_b64 s[64:65], s[64:65], vcc\n"                                                                           \
	"s_or_b64 s[58:59], s[58:59], s[64:65]\n"                                                                       \
	"s_and_b64 s[54:55], s[54:55], s[56:57]\n"                                                                      \
	"s_and_b64 s[54:55], s[54:55], s[58:59]\n"                  /* the lanes that take this hit */                  \
	"s_cbranch_scc0 L_" P "tnext_%=\n"                                                                              \
	"s_and_b32 s52, " CUROP ", 0x7fffffff\n"                    /* the triangle's row */                            \
	"v_mov_b32 v50, s52\n"                                                                                          \
	"v_mov_b32 v51, " RS##_ID "\n"                                                                                   \
	"v_cndmask_b32_e64 " MRT_OP("bt", P) ", " MRT_OP("bt", P) ", v55, s[54:55]\n"                                   \
	"v_cndmask_b32_e64 " MRT_OP("bu", P) ", " MRT_OP("bu", P) ", v58, s[54:55]\n"                                   \
	"v_cndmask_b32_e64 " MRT_OP("bv", P) ", " MRT_OP("bv", P) ", v59, s[54:55]\n"                                   \
	"v_cndmask_b32_e64 " MRT_OP("bs", P) ", " MRT_OP("bs", P) ", v50, s[54:55]\n"                                   \
	"v_cndmask_b32_e64 " MRT_OP("bi", P) ", " MRT_OP("bi", P) ", v51, s[54:55]\n"                                   \
	ANYHIT_CODE                                                                                                     \
	"L_" P "tnext_%=:\n"

// a triangle step of a 64-ray packet: the test, then the next triangle of the leaf or (last one) the pop bit in %[ev]
#define MRT_ROWS_TRI_STEP(P, RS, POPBIT, CNT_T, ANYHIT_CODE)                                                         \
	CNT_T                                                                                                           \
	MRT_ROWS_TRI_TEST(P, RS, RS##_MASK, MRT_OP("cur", P), ANYHIT_CODE)                                              \
	"s_bitcmp1_b32 " RS##_FLAGS ", 0\n"                          /* the last triangle of its leaf? */                \
	"s_cbranch_scc1 L_" P "tpop_%=\n"                                                                               \
	"s_add_u32 " MRT_OP("cur", P) ", " MRT_OP("cur", P) ", 1\n"                                                     \
	"s_branch L_" P "done_%=\n"                                                                                     \
	"L_" P "tpop_%=:\n"                                                                                             \
	"s_or_b32 %[ev], %[ev], " POPBIT "\n"

// closest hit: the new limit of an accepting lane is its t
#define MRT_ROWS_NEAREST(P) \
	"v_cndmask_b32_e64 " MRT_OP("lim", P) ", " MRT_OP("lim", P) ", v55, s[54:55]\n"
// any hit: an accepting lane is finished; when no lane of the packet is left the packet ends (sentinel, via the slow path)
#define MRT_ROWS_ANYHIT(P, DONEBIT) \
	"v_cndmask_b32_e64 " MRT_OP("lim", P) ", " MRT_OP("lim", P) ", %[vneg], s[54:55]\n"                             \
	"v_cmp_neq_f32_e64 s[56:57], " MRT_OP("lim", P) ", %[vneg]\n"                                                   \
	"s_cmp_lg_u64 s[56:57], 0\n"                                                                                    \
	"s_cbranch_scc1 L_" P "tnext_%=\n"                                                                              \
	"s_mov_b32 " MRT_OP("cur", P) ", 0x7fffffff\n"                                                                  \
	"s_or_b32 %[ev], %[ev], " DONEBIT "\n"                                                                          \
	"s_branch L_" P "done_%=\n"

// a step of packet P, whatever its current row is
#define MRT_ROWS_STEP(P, RS, POPBIT, CNT_N, CNT_T, CNT_P, ANYHIT_CODE, BX, BY, BZ)                                            \
	"s_bitcmp1_b32 " MRT_OP("cur", P) ", 31\n"                                                                      \
	"s_cbranch_scc1 L_" P "tri_%=\n"                                                                                \
	CNT_N                                                                                                           \
	MRT_ROWS_NODE_STEP(P, RS, POPBIT, CNT_P, BX, BY, BZ)                                                             \
	"s_branch L_" P "done_%=\n"                                                                                     \
	"L_" P "tri_%=:\n"                                                                                              \
	MRT_ROWS_TRI_STEP(P, RS, POPBIT, CNT_T, ANYHIT_CODE)                                                             \
	"L_" P "done_%=:\n"

// ---- the pops; the pop that fetches first (round 6; -DMRT_ROWS_POPFETCH=1, NOT the default) ------------------------------------
// Everything that switch changes stands in this section: the words the loops take from it (MRT_ROWS_TOP_*, MRT_ROWS_HAVE,
// MRT_ROWS_EXIT_WAIT) and both forms of both pops.
// Measured (profiles/r19_pop_fetch.json): 1.6 % fewer wave cycles, about 1 % of C3's kernel time in each of two
// sessions, less than the builds' own spread: the gate for a gain fails, so the default build keeps the pop that reads its entry
// first and is the same machine code as before.  The form, for whoever measures it again:
// top (s68, the first scalar above the fixed ones; the kernel has 72) shadows ONE field of the stack, which stays in the LDS entry
// for entry and byte for byte as it was.  Invariant inside each walk block: top == the ref field of the entry at sp - entry size.
// Every block is entered with an empty stack (only the sentinel below sp: rows_walks_and_records sets sp so), so top starts as
// 0x7FFFFFFF; a push copies the far ref (s53) into it: one scalar instruction.  A pop runs in this order:
//   1. cur = top; top == 0x7FFFFFFF -> leave the walk: the sentinel is never read from the LDS;
//   2. s_lshl / s_load_dwordx16 of row top into s[20:35]: the fetch is in flight from here.  Every path into a pop has finished
//      with the row registers (the leaf path tests RA_FLAGS before it branches, the miss path has made its masks);
//   3. the LDS reads: the masks of the entry popped and the ref word of the entry below it, the new top (it always exists: the
//      sentinel lies at the bottom).  DS offsets are unsigned, so the lower entry's address goes to a temporary, both reads use
//      positive offsets from it, then sp is set;
//   4. ONE s_waitcnt lgkmcnt(0): scalar loads and LDS reads share the counter, scalar loads return out of order, and the child
//      prefetches into s64 / s65 may still be on their way (the triangle test writes those registers): only 0 is safe, and it
//      covers the row, the entry and the prefetches;
//   5. v_readfirstlane of the mask words and of the new top (LDS results, behind the wait: no VALU write precedes them), and on at
//      the label BEHIND the loop head's own fetch and wait.
// So the LDS round trip and the hand-overs to the scalar unit run under the row fetch's latency instead of in front of it.  The
// any-hit early finish leaves with entries still on the stack, as before (top is dead from there).  The four-wide walk keeps the
// old pop (MRT_ROWSW_POP_READ) in either build: its loop head issues a second load by the row's kind, and it is an experiment kept
// for the record.
#ifndef MRT_ROWS_POPFETCH
#define MRT_ROWS_POPFETCH 0
#endif
#define RA_TOP "s68"
#if MRT_ROWS_POPFETCH
#define MRT_ROWS_TOP_CLOBBER "s68",
#define MRT_ROWS_TOP_EMPTY "s_mov_b32 s68, 0x7fffffff\n"   /* on entry to a block: the stack is empty, its top is the sentinel */
#define MRT_ROWS_TOP_PUSHED "s_mov_b32 s68, s53\n"         /* the entry being pushed (far ref s53) is the stack's top */
#define MRT_ROWS_HAVE "L_have_%=:\n"                       /* behind the loop head's fetch: the row is in s[20:35] */
// (the pop at the sentinel waits for nothing: no prefetch may land in s64 / s65 once the compiler owns them again)
#define MRT_ROWS_EXIT_WAIT "s_waitcnt vmcnt(0) lgkmcnt(0)\n"
#else
#define MRT_ROWS_TOP_CLOBBER
#define MRT_ROWS_TOP_EMPTY ""
#define MRT_ROWS_TOP_PUSHED ""
#define MRT_ROWS_HAVE ""
#define MRT_ROWS_EXIT_WAIT "s_waitcnt vmcnt(0)\n"
#endif

// The pop of the shared walks (32-byte entries {group A's mask, group B's mask, ref, -}) that reads its entry first: the own masks
// into M0..M3, on at RELOAD, or out through L_exit at the sentinel
#define MRT_ROWSW_POP_READ(M0, M1, M2, M3, RELOAD)                                                                    \
	"v_add_u32 %[spA], -32, %[spA]\n"                                                                               \
	"ds_read_b128 v[50:53], %[spA]\n"                                                                               \
	"ds_read_b32 v54, %[spA] offset:16\n"                                                                           \
	"s_waitcnt lgkmcnt(0)\n"                                                                                        \
	"v_readfirstlane_b32 %[curA], v54\n"                                                                            \
	"v_readfirstlane_b32 " M0 ", v50\n"                                                                             \
	"v_readfirstlane_b32 " M1 ", v51\n"                                                                             \
	"v_readfirstlane_b32 " M2 ", v52\n"                                                                             \
	"v_readfirstlane_b32 " M3 ", v53\n"                                                                             \
	"s_cmp_lg_u32 %[curA], 0x7fffffff\n"                                                                            \
	"s_cbranch_scc1 " RELOAD "\n"                                                                                   \
	"s_branch L_exit_%=\n"

// MRT_ROWS_POP1: the pop of the one-packet loop (16-byte entries {ref, -, mask}), entered with an event in %[ev]: the pop bit (bit 0),
// or the any-hit finish (cur is the sentinel already).  Falls out at the end of the walk; else goes on at L_loop, or (fetching first)
// at L_have.
// MRT_ROWSW_POP: the pop of the two 128-ray loops: leaves through L_exit at the sentinel.  WITH_FETCH: what the culling loop issues
// beside the popped row's scalar fetch (the vector copy of the row); RELOAD: the label the pop that reads its entry first goes on at
// (the loop head, or the culling loop's request for that copy in front of it).
#if MRT_ROWS_POPFETCH
// "the pop" above: cur = top, out at the sentinel, the fetch of row top (T_PRE / T_POST: the counting builds' clock), the popped
// entry's mask into v[52:53] and the ref of the entry below it into v50 under it, one wait, three hand-overs
#define MRT_ROWS_POP1(T_PRE, T_POST)                                                                                \
	"s_bitcmp1_b32 %[ev], 0\n"                                                                                      \
	"s_mov_b32 %[ev], 0\n"                                                                                          \
	"s_cbranch_scc0 L_exit_%=\n"                                                                                    \
	"s_mov_b32 %[curA], " RA_TOP "\n"                                                                               \
	"s_cmp_eq_u32 " RA_TOP ", 0x7fffffff\n"                                                                         \
	"s_cbranch_scc1 L_exit_%=\n"                                                                                    \
	"s_lshl_b32 s52, " RA_TOP ", 6\n"                                                                               \
	T_PRE                                                                                                           \
	"s_load_dwordx16 s[20:35], %[rows], s52\n"                                                                      \
	"v_add_u32 v50, -32, %[spA]\n"                           /* the entry below the one popped */                  \
	"ds_read_b64 v[52:53], v50 offset:24\n"                                                                         \
	"ds_read_b32 v50, v50\n"                                                                                        \
	"v_add_u32 %[spA], -16, %[spA]\n"                                                                               \
	"s_waitcnt lgkmcnt(0)\n"                                                                                        \
	T_POST                                                                                                          \
	"v_readfirstlane_b32 s60, v52\n"                                                                                \
	"v_readfirstlane_b32 s61, v53\n"                                                                                \
	"v_readfirstlane_b32 " RA_TOP ", v50\n"                                                                         \
	"s_branch L_have_%=\n"                                                                                          \
	"L_exit_%=:\n"
// "the pop" above: goes on at L_have with the popped row in s[20:35], its masks in s[60:63], cur = its ref, top = the ref of the entry below
#define MRT_ROWSW_POP(WITH_FETCH, RELOAD)                                                                             \
	"s_mov_b32 %[curA], " RA_TOP "\n"                                                                               \
	"s_cmp_eq_u32 " RA_TOP ", 0x7fffffff\n"                                                                         \
	"s_cbranch_scc1 L_exit_%=\n"                                                                                    \
	"s_lshl_b32 s52, " RA_TOP ", 6\n"                                                                               \
	"s_load_dwordx16 s[20:35], %[rows], s52\n"                                                                      \
	WITH_FETCH                                                                                                      \
	"v_add_u32 v54, -64, %[spA]\n"                            /* the entry below the one popped */                  \
	"ds_read_b128 v[50:53], v54 offset:32\n"                                                                        \
	"ds_read_b32 v54, v54 offset:16\n"                                                                              \
	"v_add_u32 %[spA], -32, %[spA]\n"                                                                               \
	"s_waitcnt lgkmcnt(0)\n"                                                                                        \
	"v_readfirstlane_b32 s60, v50\n"                                                                                \
	"v_readfirstlane_b32 s61, v51\n"                                                                                \
	"v_readfirstlane_b32 s62, v52\n"                                                                                \
	"v_readfirstlane_b32 s63, v53\n"                                                                                \
	"v_readfirstlane_b32 " RA_TOP ", v54\n"                                                                         \
	"s_branch L_have_%=\n"
#else
#define MRT_ROWS_POP1(T_PRE, T_POST)                                                                              \
	"s_bitcmp1_b32 %[ev], 0\n"                                                                                      \
	"s_cbranch_scc0 L_Api_%=\n"                                                                                     \
	"v_add_u32 %[spA], -16, %[spA]\n"                                                                               \
	"ds_read_b128 v[50:53], %[spA]\n"                                                                               \
	"L_Api_%=:\n"                                                                                                   \
	"s_waitcnt lgkmcnt(0)\n"                                                                                        \
	"s_bitcmp1_b32 %[ev], 0\n"                                                                                      \
	"s_cbranch_scc0 L_Apt_%=\n"                                                                                     \
	"v_readfirstlane_b32 %[curA], v50\n"                                                                            \
	"v_readfirstlane_b32 s60, v52\n"                                                                                \
	"v_readfirstlane_b32 s61, v53\n"                                                                                \
	"L_Apt_%=:\n"                                                                                                   \
	"s_mov_b32 %[ev], 0\n"                                                                                          \
	"s_cmp_lg_u32 %[curA], 0x7fffffff\n"                                                                            \
	"s_cbranch_scc1 L_loop_%=\n"
#define MRT_ROWSW_POP(WITH_FETCH, RELOAD) MRT_ROWSW_POP_READ("s60", "s61", "s62", "s63", RELOAD)
#endif

#define MRT_ROWS_CLOBBERS                                                                                             \
	"vcc", "scc", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "s30", "s31", "s32", "s33", \
	"s34", "s35", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", \
	"s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", \
	"s66", "s67", MRT_ROWS_TOP_CLOBBER "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60"

// operands of one packet (S = its PacketRegs)
#define MRT_ROWS_OUT(P, S)                                                                                            \
	[cur##P] "+s"(S.cur), [sp##P] "+v"(S.sp), [lim##P] "+v"(S.lim), [bt##P] "+v"(S.bt), [bu##P] "+v"(S.bu),         \
	[bv##P] "+v"(S.bv), [bs##P] "+v"(S.bs), [bi##P] "+v"(S.bi), [mask##P] "+s"(S.mask)
#define MRT_ROWS_IN(P, S)                                                                                             \
	[ox##P] "v"(S.ox), [oy##P] "v"(S.oy), [oz##P] "v"(S.oz), [dx##P] "v"(S.dx), [dy##P] "v"(S.dy), [dz##P] "v"(S.dz), \
	[tmin##P] "v"(S.tmin), [ix##P] "v"(S.ix), [iy##P] "v"(S.iy), [iz##P] "v"(S.iz), [nrx##P] "v"(S.nrx),            \
	[nry##P] "v"(S.nry), [nrz##P] "v"(S.nrz)

// everything a packet's walk holds in registers
struct PacketRegs {
	float ox, oy, oz, dx, dy, dz, tmin;   // the ray (t_max lives on in lim / bt)
	float ix, iy, iz, nrx, nry, nrz;      // safe_inv(d), -(o * inv)
	float lim;                            // far limit of the box tests: best_t, or -FLT_MAX for a lane that takes no part
	float bt, bu, bv;                     // best hit
	uint32_t bs, bi;                      // its row (0xFFFFFFFF = none) and triangle id
	uint32_t sp;                          // LDS byte address of the next free stack entry
	uint32_t cur;                         // wave-uniform: the row to visit next (bit 31: a triangle), 0x7FFFFFFF = finished
	unsigned long long mask;              // wave-uniform: the lanes that own the current row (matters for triangles)
};

// ---- the loops ------------------------------------------------------------------------------------------------
// One packet (register set A).  In: cur = a row to visit.  Out: cur = 0x7FFFFFFF.
#define MRT_ROWS_LOOP1(CNT_N, CNT_T, CNT_P, T_PRE, T_POST, ANYHIT_CODE, BX, BY, BZ)                                          \
	asm volatile(                                                                                                   \
		"s_mov_b64 s[60:61], %[maskA]\n"                                                                            \
		MRT_ROWS_TOP_EMPTY \
		"L_loop_%=:\n"                                                                                              \
		"s_lshl_b32 s52, %[curA], 6\n"                                                                              \
		T_PRE                                                                                                       \
		"s_load_dwordx16 s[20:35], %[rows], s52\n"                                                                  \
		"s_waitcnt lgkmcnt(0)\n"                                                                                    \
		T_POST                                                                                                      \
		MRT_ROWS_HAVE \
		MRT_ROWS_STEP("A", RA, "1", CNT_N, CNT_T, CNT_P, ANYHIT_CODE, BX, BY, BZ)                                   \
		"s_cmp_eq_u32 %[ev], 0\n"                                                                                   \
		"s_cbranch_scc1 L_loop_%=\n"                                                                                \
		MRT_ROWS_POP1(T_PRE, T_POST)                                                                                \
		"s_waitcnt vmcnt(0)\n"               /* no prefetch may land in v60 once the compiler owns it again */     \
		"s_mov_b64 %[maskA], s[60:61]\n"                                                                            \
		: MRT_ROWS_OUT(A, a), [ev] "+s"(ev), [cntn] "+s"(cnt_n), [cntt] "+s"(cnt_t), [cntw] "+s"(cnt_w), [cntp] "+s"(sp_max) \
		: MRT_ROWS_IN(A, a), [rows] "s"(rows), [qmask] "s"(qmask), [eps] "s"(eps), [vneg] "v"(vneg)                 \
		: MRT_ROWS_CLOBBERS)

// ---- owner-narrowed EXEC in the paired walk (round 8; -DMRT_ROWS_OWNEXEC=1, NOT the default) -----------------------------------
// Everything that switch changes stands in this section: the words MRT_ROWS_LOOPW takes from it.  Switch off, they are empty and
// the build is the parent's machine code.
// What it does: a group's box test and its triangle test run with EXEC = the lanes of the group that own the row, where the
// parent runs them on all 64.  The parent is correct without any masking (a lane that missed an ancestor's box cannot pass a
// child's: the planes are monotone, and lim is -FLT_MAX for a lane that takes no part), so the masks that come out are the same
// bits: a v_cmp_e64 under a narrowed EXEC writes 0 for the lanes that are off, which is what those lanes produce today.
//   * node step: EXEC = the group's own mask OR lane 0, in front of MRT_ROWS_SLAB and its two v_cmp.  Lane 0 keeps v50 / v56 (tl /
//     tr of the group tested last) current in the lane MRT_ROWSW_DECIDE reads, so the near / far order and every counter of the
//     counting builds stay the parent's.  Lane 0 takes part only if it was in the EXEC the block was entered with;
//   * triangle test: EXEC = the group's own mask: the v_div_scale / v_div_fmas VCC chain, the v_cndmask updates and the any-hit
//     code run on owners only;
//   * EXEC is the entry EXEC again, one s_mov_b64 per step, before anything that is not a per-lane test: MRT_ROWSW_DECIDE (its
//     v_add_u32 on sp must run on every lane), the pops and their v_readfirstlane, the any-hit finish (MRT_ROWSW_ANYDONE compares
//     every lane's lim), the counting macros, the exit.  The child prefetches are scalar and stand in front of the tests.
// The two copies of the walk take different words, because the kernel has no scalar register to spare (with four more fixed ones
// the compiler spilled scalars to lanes on the whole-tile path):
//   * whole-tile fast path (rows_walk_wide_whole): entered with EXEC all ones, so lane 0 is the constant 1 and the constant -1
//     restores: one scalar instruction per group tested, one per step, no register;
//   * general code (rows_walk_wide): the entry EXEC is kept in s[70:71] (the last pair below the compiler's registers; s68 is the
//     stack's top in MRT_ROWS_POPFETCH builds), and an s_and_b64 with it follows the OR with lane 0: two per group tested.
// gfx950 wait states after a scalar write of EXEC: a VALU instruction that only executes under it needs none (the hardware
// interlocks), nor does v_readfirstlane after the restoring s_mov_b64; a DPP instruction needs five wait states, and the paired walk
// has none (the culling loop has its DPP sums, one reason it would pay more for this).  A lane mask written by v_cmp_e64 under a
// narrowed EXEC goes to the scalar ALU as before.
// The culling loop (MRT_ROWS_LOOPC), the one-packet loop (MRT_ROWS_LOOP1) and the four-wide walk keep the parent's text in either build.
#ifndef MRT_ROWS_OWNEXEC
#define MRT_ROWS_OWNEXEC 0
#endif
// the words of a copy of the walk: on entry, behind the OR with lane 0, the restore, and the name of its clobbers
#if MRT_ROWS_OWNEXEC
#define MRT_ROWS_OWN_WHOLE "", "", "s_mov_b64 exec, -1\n", WHOLE
#define MRT_ROWS_OWN_ANYEXEC "s_mov_b64 s[70:71], exec\n", "s_and_b64 exec, exec, s[70:71]\n", "s_mov_b64 exec, s[70:71]\n", ANYEXEC
#define MRT_ROWS_OWN_CLOBBER_WHOLE
#define MRT_ROWS_OWN_CLOBBER_ANYEXEC "s70", "s71",
#define MRT_ROWS_OWN_NODE(OWN, KEEP) "s_or_b64 exec, " OWN ", 1\n" KEEP
#define MRT_ROWS_OWN_LEAF(OWN) "s_mov_b64 exec, " OWN "\n"
#else
#define MRT_ROWS_OWN_WHOLE "", "", "", WHOLE
#define MRT_ROWS_OWN_ANYEXEC "", "", "", ANYEXEC
#define MRT_ROWS_OWN_CLOBBER_WHOLE
#define MRT_ROWS_OWN_CLOBBER_ANYEXEC
#define MRT_ROWS_OWN_NODE(OWN, KEEP) ""
#define MRT_ROWS_OWN_LEAF(OWN) ""
#endif

// ---- the 128-ray packet: groups A and B (two rays per lane) share one walk --------------------------------------
// One group's slab test at a node row, skipped (no child hit) when no lane of the group owns the node.
// LM / RM: the group's lanes that hit the left / right child.  v50 / v56 keep tl / tr of the last group tested.
#define MRT_ROWSW_GROUP_SLAB(P, OWN, LM, RM, BX, BY, BZ, NARROW)                                                           \
	"s_cmp_eq_u64 " OWN ", 0\n"                                                                                     \
	"s_cbranch_scc1 L_" P "skip_%=\n"         /* (out of line: the common path falls through) */                    \
	NARROW                                                                                                          \
	MRT_ROWS_SLAB(P, RA, BX, BY, BZ)                                                                                \
	"v_cmp_le_f32_e64 " LM ", v50, v53\n"                                                                           \
	"v_cmp_le_f32_e64 " RM ", v56, v52\n"                                                                           \
	"L_" P "sdone_%=:\n"
#define MRT_ROWSW_GROUP_SKIP(P, LM, RM)                                                                               \
	"L_" P "skip_%=:\n"                                                                                             \
	"s_mov_b64 " LM ", 0\n"                                                                                         \
	"s_mov_b64 " RM ", 0\n"                                                                                         \
	"s_branch L_" P "sdone_%=\n"

// any hit in the 128-ray walk: an accepting lane is finished; the walk ends when no lane of either group is left
#define MRT_ROWSW_ANYHIT(P) \
	"v_cndmask_b32_e64 " MRT_OP("lim", P) ", " MRT_OP("lim", P) ", %[vneg], s[54:55]\n"
#define MRT_ROWSW_ANYDONE                                                                                             \
	"v_cmp_neq_f32_e64 s[56:57], %[limA], %[vneg]\n"                                                                \
	"v_cmp_neq_f32_e64 s[58:59], %[limB], %[vneg]\n"                                                                \
	"s_or_b64 s[56:57], s[56:57], s[58:59]\n"                                                                       \
	"s_cbranch_scc1 L_goon_%=\n"                                                                                    \
	"s_mov_b32 %[curA], 0x7fffffff\n"                                                                               \
	"s_branch L_exit_%=\n"                                                                                          \
	"L_goon_%=:\n"

// Both child rows are pulled into the scalar cache as soon as the node's own row has arrived, before the slab tests:
// the row fetch of the next step (whichever child it visits) then finds its line there instead of waiting for the L2
// (two one-dword scalar loads into the triangle test's temporaries s64 / s65, which nothing reads; they are long back
// when the next step waits on lgkmcnt).  (The far-child vector prefetch of round 1 that this replaced, and the same two loads
// tried inside the culling loop, are measured in DESIGN 4.1c / 4.1d and profiles/r03_kprefetch_pmc.txt.)
#define MRT_ROWSW_KPREFETCH                                                                                           \
	"s_lshl_b32 s48, " RA_LREF ", 6\n"                                                                               \
	"s_lshl_b32 s49, " RA_RREF ", 6\n"                                                                               \
	"s_load_dword s64, %[rows], s48\n"                                                                              \
	"s_load_dword s65, %[rows], s49\n"

// ---- the steps the two 128-ray loops share, and the four-wide loop where it does the same ---------------------------------------
// The near / far decision from the groups' hit masks (s[36:43]; tl / tr of the group tested last in v50 / v56) and the push of the
// far child: the next row's ref into cur, its own masks into s[60:63], then on at L_loop; no child hit: L_pop.  The far child's two
// masks (s[50:51], s[58:59]) and its ref (s53) go to v50..v54 for the two ds_writes (gfx950 moves a scalar pair in one v_mov_b64).
// COPY_NEAR / COPY_L / COPY_R: the culling loop's note of which vector copy the next row has, where both children / the left one /
// the right one was hit.
#define MRT_ROWSW_DECIDE(CNT_P, COPY_NEAR, COPY_L, COPY_R)                                                            \
	"s_or_b64 s[44:45], s[36:37], s[40:41]\n"    /* any lane of the 128 hit the left child?  */                     \
	"s_cbranch_scc0 L_lmiss_%=\n"                                                                                   \
	"s_or_b64 vcc, s[38:39], s[42:43]\n"         /* ... the right child? */                                         \
	"s_cbranch_scc0 L_onlyl_%=\n"                                                                                   \
	/* both: lane 0 of the group tested last (its tl, tr are still in v50, v56) decides which is nearer */          \
	"v_cmp_lt_f32_e64 s[46:47], v50, v56\n"      /* (order = speed only) */                                         \
	"s_bitcmp1_b32 s46, 0\n"                                                                                        \
	"s_cselect_b32 s53, " RA_RREF ", " RA_LREF "\n"       /* far  */                                                \
	"s_cselect_b32 %[curA], " RA_LREF ", " RA_RREF "\n"   /* near */                                                \
	"s_cselect_b64 s[50:51], s[38:39], s[36:37]\n"        /* the far child's masks: group A, group B */             \
	"s_cselect_b64 s[58:59], s[42:43], s[40:41]\n"                                                                  \
	"s_cselect_b64 s[60:61], s[36:37], s[38:39]\n"        /* the near child's */                                    \
	"s_cselect_b64 s[62:63], s[40:41], s[42:43]\n"                                                                  \
	COPY_NEAR                                                                                                       \
	MRT_ROWS_TOP_PUSHED                                                                                             \
	"v_mov_b64 v[50:51], s[50:51]\n"                                                                                \
	"v_mov_b64 v[52:53], s[58:59]\n"                                                                                \
	"v_mov_b32 v54, s53\n"                                                                                          \
	"ds_write_b128 %[spA], v[50:53]\n"                                                                              \
	"ds_write_b32 %[spA], v54 offset:16\n"                                                                          \
	"v_add_u32 %[spA], 32, %[spA]\n"                                                                                \
	CNT_P                                                                                                           \
	"s_branch L_loop_%=\n"                                                                                          \
	"L_onlyl_%=:\n"                                                                                                 \
	"s_mov_b32 %[curA], " RA_LREF "\n"                                                                              \
	"s_mov_b64 s[60:61], s[36:37]\n"                                                                                \
	"s_mov_b64 s[62:63], s[40:41]\n"                                                                                \
	COPY_L                                                                                                          \
	"s_branch L_loop_%=\n"                                                                                          \
	"L_lmiss_%=:\n"                                                                                                 \
	"s_or_b64 vcc, s[38:39], s[42:43]\n"                                                                            \
	"s_cbranch_scc0 L_pop_%=\n"                                                                                     \
	"s_mov_b32 %[curA], " RA_RREF "\n"                                                                              \
	"s_mov_b64 s[60:61], s[38:39]\n"                                                                                \
	"s_mov_b64 s[62:63], s[42:43]\n"                                                                                \
	COPY_R                                                                                                          \
	"s_branch L_loop_%=\n"

// The leaf section: the triangle row in s[20:35] against each group that has a lane owning it (OWN_A / OWN_B), then the leaf's next
// triangle (on at L_loop) or, after its last one, the pop (L_pop).  ARRIVED: what a loop that comes here with the row
// still on its way puts first.  NARROW_A / NARROW_B / RESTORE: the words of MRT_ROWS_OWNEXEC in the loop that takes them, else "".
#define MRT_ROWSW_LEAF(OWN_A, OWN_B, ARRIVED, CNT_T, ANYA, ANYB, ANYDONE, NARROW_A, NARROW_B, RESTORE)                 \
	"L_tri_%=:\n"                                                                                                   \
	CNT_T                                                                                                           \
	ARRIVED                                                                                                         \
	"s_cmp_eq_u64 " OWN_A ", 0\n"                                                                                   \
	"s_cbranch_scc1 L_Atnext_%=\n"                                                                                  \
	NARROW_A                                                                                                        \
	MRT_ROWS_TRI_TEST("A", RA, OWN_A, "%[curA]", ANYA)                                                              \
	"s_cmp_eq_u64 " OWN_B ", 0\n"                                                                                   \
	"s_cbranch_scc1 L_Btnext_%=\n"                                                                                  \
	NARROW_B                                                                                                        \
	MRT_ROWS_TRI_TEST("B", RA, OWN_B, "%[curA]", ANYB)                                                              \
	RESTORE                                                                                                         \
	ANYDONE                                                                                                         \
	"s_bitcmp1_b32 " RA_FLAGS ", 0\n"        /* the last triangle of its leaf? */                                   \
	"s_cbranch_scc1 L_pop_%=\n"                                                                                     \
	"s_add_u32 %[curA], %[curA], 1\n"                                                                               \
	"s_branch L_loop_%=\n"

// The exit: WAIT (nothing in flight may land in a register once the compiler owns it again), the own masks back to their operands
#define MRT_ROWSW_EXIT(WAIT, OWN_A, OWN_B)                                                                            \
	"L_exit_%=:\n"                                                                                                  \
	WAIT                                                                                                            \
	"s_mov_b64 %[maskA], " OWN_A "\n"                                                                               \
	"s_mov_b64 %[maskB], " OWN_B "\n"

// what a paired walk hands back: group A's packet whole, of group B's what is not shared, the counters
#define MRT_ROWSW_OUT                                                                                                 \
	MRT_ROWS_OUT(A, a), [limB] "+v"(b.lim), [btB] "+v"(b.bt), [buB] "+v"(b.bu), [bvB] "+v"(b.bv),                   \
	[bsB] "+v"(b.bs), [biB] "+v"(b.bi), [maskB] "+s"(b.mask), [cntn] "+s"(cnt_n), [cntt] "+s"(cnt_t), [cntp] "+s"(sp_max)

// ---- the packed node step (round 7; -DMRT_ROWS_PKSLAB=1, NOT the default) ------------------------------------------------------
// Measured (profiles/r20_packed_slab.json): 16 % fewer vector instructions per wave at C3 (9 618 -> 8 067) and
// the kernel 6 % SLOWER (1.66 -> 1.76 ms, well outside both builds' spread): in this walk a v_pk_fma_f32 costs more than the two
// v_fma_f32 it stands for.  So the default build keeps the two single-group tests and is the same machine code as before.  The form,
// for whoever measures it again:
// On a row that BOTH groups own, MRT_ROWS_SLAB multiplies the same twelve plane scalars first into group A's six registers and then
// into group B's: 24 v_fma_f32.  v_pk_fma_f32 does an {A, B} pair in one instruction (the same IEEE fma per component: the same
// bits), so such a row costs 12 packed fmas + 2 x 10 (four clamps, max3 / min3 twice, four compares) = 32 vector instructions
// where 44 stood.  For that the six hot values of the two groups stand side by side in aligned register pairs,
//   ix v[12:13]  iy v[14:15]  iz v[16:17]  nrx v[18:19]  nry v[20:21]  nrz v[22:23]      (low half group A, high half group B),
// which the operands of MRT_ROWS_LOOPW are pinned to (MRT_ROWSW_IN_A / _B); every single-group test still names its half through
// its operand (%[ixA] is v12), so MRT_ROWS_SLAB and the triangle test are the text they were.  (Where the pairs stand was chosen
// by compiling: at v[38:49] the headline's general code spilled 12 bytes to scratch, at v[12:23] every instantiation has the
// parent's registers, scratch and occupancy.)  A plane scalar is read from its aligned pair of s[20:35], op_sel / op_sel_hi
// choosing the half for both components: one SGPR source per instruction.
// Temporaries: v50..v60 as they stand (five pairs and v60; a box's six products are never all live at once: the left box's far z
// and the right box's products take the registers its near planes have left); no instruction reads its predecessor's result.
// It ends as the single tests do: group B (the group tested last) leaves tl in v50 and tr in v56 for the near / far decision, the
// masks are in s[36:43].  A row only one group owns takes MRT_ROWSW_GROUP_SLAB, out of line.
// The culling loop (MRT_ROWS_LOOPC) keeps its one-box tests in either build: v61 / v62 hold its row copies there, and a culled box
// leaves a step with one box for two groups, half of what a packed step pairs up.
#ifndef MRT_ROWS_PKSLAB
#define MRT_ROWS_PKSLAB 0
#endif
// a plane's aligned scalar pair and the half it is
#define RA_LMINX_PK "s[20:21]", "0"
#define RA_LMINY_PK "s[20:21]", "1"
#define RA_LMINZ_PK "s[22:23]", "0"
#define RA_LMAXX_PK "s[24:25]", "0"
#define RA_LMAXY_PK "s[24:25]", "1"
#define RA_LMAXZ_PK "s[26:27]", "0"
#define RA_RMINX_PK "s[28:29]", "0"
#define RA_RMINY_PK "s[28:29]", "1"
#define RA_RMINZ_PK "s[30:31]", "0"
#define RA_RMAXX_PK "s[32:33]", "0"
#define RA_RMAXY_PK "s[32:33]", "1"
#define RA_RMAXZ_PK "s[34:35]", "0"
#define MRT_NEARPK_0(RS, AX, SIDE) RS##_##SIDE##MIN##AX##_PK
#define MRT_NEARPK_1(RS, AX, SIDE) RS##_##SIDE##MAX##AX##_PK
#define MRT_FARPK_0(RS, AX, SIDE) RS##_##SIDE##MAX##AX##_PK
#define MRT_FARPK_1(RS, AX, SIDE) RS##_##SIDE##MIN##AX##_PK
#ifndef MRT_PK_V0
#define MRT_PK_V0 12
#define MRT_PK_V1 13
#define MRT_PK_V2 14
#define MRT_PK_V3 15
#define MRT_PK_V4 16
#define MRT_PK_V5 17
#define MRT_PK_V6 18
#define MRT_PK_V7 19
#define MRT_PK_V8 20
#define MRT_PK_V9 21
#define MRT_PK_V10 22
#define MRT_PK_V11 23
#endif
#define MRT_STR2(X) #X
#define MRT_STR(X) MRT_STR2(X)
#define MRT_PK_PAIR(LO, HI) "v[" MRT_STR(LO) ":" MRT_STR(HI) "]"
#define MRT_PK_PIN(N) "{v" MRT_STR(N) "}"
#define MRT_PK_IX MRT_PK_PAIR(MRT_PK_V0, MRT_PK_V1)
#define MRT_PK_IY MRT_PK_PAIR(MRT_PK_V2, MRT_PK_V3)
#define MRT_PK_IZ MRT_PK_PAIR(MRT_PK_V4, MRT_PK_V5)
#define MRT_PK_NRX MRT_PK_PAIR(MRT_PK_V6, MRT_PK_V7)
#define MRT_PK_NRY MRT_PK_PAIR(MRT_PK_V8, MRT_PK_V9)
#define MRT_PK_NRZ MRT_PK_PAIR(MRT_PK_V10, MRT_PK_V11)
// DST = {plane * inv + nr of group A, of group B}
#define MRT_PKFMA2(DST, PAIR, HALF, INV, NR)                                                                          \
	"v_pk_fma_f32 " DST ", " PAIR ", " INV ", " NR " op_sel:[" HALF ",0,0] op_sel_hi:[" HALF ",1,1]\n"
#define MRT_PKFMA(DST, PLANE, INV, NR) MRT_PKFMA2(DST, PLANE, INV, NR)
#define MRT_ROWSW_PKSLAB(BX, BY, BZ)                                                                                  \
	MRT_PKFMA("v[50:51]", MRT_NEARPK_##BX(RA, X, L), MRT_PK_IX, MRT_PK_NRX)                                        \
	MRT_PKFMA("v[52:53]", MRT_NEARPK_##BY(RA, Y, L), MRT_PK_IY, MRT_PK_NRY)                                        \
	MRT_PKFMA("v[54:55]", MRT_NEARPK_##BZ(RA, Z, L), MRT_PK_IZ, MRT_PK_NRZ)                                        \
	MRT_PKFMA("v[56:57]", MRT_FARPK_##BX(RA, X, L), MRT_PK_IX, MRT_PK_NRX)                                         \
	MRT_PKFMA("v[58:59]", MRT_FARPK_##BY(RA, Y, L), MRT_PK_IY, MRT_PK_NRY)                                         \
	"v_max_f32 v54, v54, %[tminA]\n"                                                                               \
	"v_max_f32 v55, v55, %[tminB]\n"                                                                               \
	"v_max3_f32 v60, v50, v52, v54\n"        /* v60 = tl of group A  */                                            \
	"v_max3_f32 v50, v51, v53, v55\n"        /* v50 = tl of group B (stays) */                                     \
	MRT_PKFMA("v[52:53]", MRT_FARPK_##BZ(RA, Z, L), MRT_PK_IZ, MRT_PK_NRZ)                                         \
	MRT_PKFMA("v[54:55]", MRT_NEARPK_##BX(RA, X, R), MRT_PK_IX, MRT_PK_NRX)                                        \
	"v_min_f32 v52, v52, %[limA]\n"                                                                                \
	"v_min_f32 v53, v53, %[limB]\n"                                                                                \
	"v_min3_f32 v56, v56, v58, v52\n"        /* v56 = tlx of group A */                                            \
	"v_min3_f32 v57, v57, v59, v53\n"        /* v57 = tlx of group B */                                            \
	MRT_PKFMA("v[52:53]", MRT_NEARPK_##BY(RA, Y, R), MRT_PK_IY, MRT_PK_NRY)                                        \
	MRT_PKFMA("v[58:59]", MRT_NEARPK_##BZ(RA, Z, R), MRT_PK_IZ, MRT_PK_NRZ)                                        \
	"v_cmp_le_f32_e64 s[36:37], v60, v56\n"  /* group A's lanes that hit the left child */                         \
	"v_cmp_le_f32_e64 s[40:41], v50, v57\n"  /* group B's */                                                       \
	"v_max_f32 v58, v58, %[tminA]\n"                                                                               \
	"v_max_f32 v59, v59, %[tminB]\n"                                                                               \
	"v_max3_f32 v60, v54, v52, v58\n"        /* v60 = tr of group A  */                                            \
	"v_max3_f32 v56, v55, v53, v59\n"        /* v56 = tr of group B (stays) */                                     \
	MRT_PKFMA("v[52:53]", MRT_FARPK_##BX(RA, X, R), MRT_PK_IX, MRT_PK_NRX)                                         \
	MRT_PKFMA("v[54:55]", MRT_FARPK_##BZ(RA, Z, R), MRT_PK_IZ, MRT_PK_NRZ)                                         \
	MRT_PKFMA("v[58:59]", MRT_FARPK_##BY(RA, Y, R), MRT_PK_IY, MRT_PK_NRY)                                         \
	"v_min_f32 v54, v54, %[limA]\n"                                                                                \
	"v_min_f32 v55, v55, %[limB]\n"                                                                                \
	"v_min3_f32 v52, v52, v58, v54\n"        /* v52 = trx of group A */                                            \
	"v_min3_f32 v53, v53, v59, v55\n"        /* v53 = trx of group B */                                            \
	"v_cmp_le_f32_e64 s[38:39], v60, v52\n"  /* group A's lanes that hit the right child */                        \
	"v_cmp_le_f32_e64 s[42:43], v56, v53\n"  /* group B's */
#if MRT_ROWS_PKSLAB
// both groups' tests at a node row, and what of them stands out of line (behind the pop)
#define MRT_ROWSW_SLABS(BX, BY, BZ, KEEP)                                                                              \
	"s_cmp_eq_u64 s[60:61], 0\n"                                                                                    \
	"s_cbranch_scc1 L_Askip_%=\n"             /* group B alone: on at L_Asdone, group B's own test */                \
	"s_cmp_eq_u64 s[62:63], 0\n"                                                                                    \
	"s_cbranch_scc1 L_single_%=\n"            /* group A alone */                                                    \
	MRT_ROWSW_PKSLAB(BX, BY, BZ)                                                                                    \
	"L_slabbed_%=:\n"
#define MRT_ROWSW_SLABS_OOL(BX, BY, BZ, KEEP)                                                                          \
	"L_single_%=:\n"                                                                                                \
	MRT_ROWSW_GROUP_SLAB("A", "s[60:61]", "s[36:37]", "s[38:39]", BX, BY, BZ, MRT_ROWS_OWN_NODE("s[60:61]", KEEP))  \
	MRT_ROWSW_GROUP_SLAB("B", "s[62:63]", "s[40:41]", "s[42:43]", BX, BY, BZ, MRT_ROWS_OWN_NODE("s[62:63]", KEEP))  \
	"s_branch L_slabbed_%=\n"                                                                                       \
	MRT_ROWSW_GROUP_SKIP("A", "s[36:37]", "s[38:39]")                                                               \
	MRT_ROWSW_GROUP_SKIP("B", "s[40:41]", "s[42:43]")
// the operands of MRT_ROWS_IN with the six hot ones pinned to their halves of the pairs above
#define MRT_ROWSW_IN_A(S)                                                                                             \
	[oxA] "v"(S.ox), [oyA] "v"(S.oy), [ozA] "v"(S.oz), [dxA] "v"(S.dx), [dyA] "v"(S.dy), [dzA] "v"(S.dz),            \
	[tminA] "v"(S.tmin), [ixA] MRT_PK_PIN(MRT_PK_V0)(S.ix), [iyA] MRT_PK_PIN(MRT_PK_V2)(S.iy), [izA] MRT_PK_PIN(MRT_PK_V4)(S.iz), [nrxA] MRT_PK_PIN(MRT_PK_V6)(S.nrx),      \
	[nryA] MRT_PK_PIN(MRT_PK_V8)(S.nry), [nrzA] MRT_PK_PIN(MRT_PK_V10)(S.nrz)
#define MRT_ROWSW_IN_B(S)                                                                                             \
	[oxB] "v"(S.ox), [oyB] "v"(S.oy), [ozB] "v"(S.oz), [dxB] "v"(S.dx), [dyB] "v"(S.dy), [dzB] "v"(S.dz),            \
	[tminB] "v"(S.tmin), [ixB] MRT_PK_PIN(MRT_PK_V1)(S.ix), [iyB] MRT_PK_PIN(MRT_PK_V3)(S.iy), [izB] MRT_PK_PIN(MRT_PK_V5)(S.iz), [nrxB] MRT_PK_PIN(MRT_PK_V7)(S.nrx),      \
	[nryB] MRT_PK_PIN(MRT_PK_V9)(S.nry), [nrzB] MRT_PK_PIN(MRT_PK_V11)(S.nrz)
#else
#define MRT_ROWSW_SLABS(BX, BY, BZ, KEEP)                                                                              \
	MRT_ROWSW_GROUP_SLAB("A", "s[60:61]", "s[36:37]", "s[38:39]", BX, BY, BZ, MRT_ROWS_OWN_NODE("s[60:61]", KEEP))  \
	MRT_ROWSW_GROUP_SLAB("B", "s[62:63]", "s[40:41]", "s[42:43]", BX, BY, BZ, MRT_ROWS_OWN_NODE("s[62:63]", KEEP))
#define MRT_ROWSW_SLABS_OOL(BX, BY, BZ, KEEP)                                                                          \
	MRT_ROWSW_GROUP_SKIP("A", "s[36:37]", "s[38:39]")                                                               \
	MRT_ROWSW_GROUP_SKIP("B", "s[40:41]", "s[42:43]")
#define MRT_ROWSW_IN_A(S) MRT_ROWS_IN(A, S)
#define MRT_ROWSW_IN_B(S) MRT_ROWS_IN(B, S)
#endif

// In: cur (group A's operand) = a row to visit, the groups' own masks.  Out: cur = 0x7FFFFFFF.
// Stack entries are 32 bytes: {group A's mask, group B's mask, ref, -}; the sentinel entry has ref 0x7FFFFFFF.
// (OWN_ENTER, OWN_KEEP, OWN_RESTORE, OWN_WHICH: the words of MRT_ROWS_OWNEXEC for this copy of the walk)
#define MRT_ROWS_LOOPW_X(CNT_N, CNT_T, CNT_P, ANYA, ANYB, ANYDONE, BX, BY, BZ, OWN_ENTER, OWN_KEEP, OWN_RESTORE, OWN_WHICH)  \
	asm volatile(                                                                                                   \
		"s_mov_b64 s[60:61], %[maskA]\n"                                                                            \
		"s_mov_b64 s[62:63], %[maskB]\n"                                                                            \
		MRT_ROWS_TOP_EMPTY \
		OWN_ENTER \
		"L_loop_%=:\n"                                                                                              \
		"s_lshl_b32 s52, %[curA], 6\n"                                                                              \
		"s_load_dwordx16 s[20:35], %[rows], s52\n"                                                                  \
		"s_waitcnt lgkmcnt(0)\n"                                                                                    \
		MRT_ROWS_HAVE \
		"s_bitcmp1_b32 %[curA], 31\n"                                                                               \
		"s_cbranch_scc1 L_tri_%=\n"                                                                                 \
		CNT_N                                                                                                       \
		MRT_ROWSW_KPREFETCH                                                                                         \
		MRT_ROWSW_SLABS(BX, BY, BZ, OWN_KEEP)                                                                       \
		OWN_RESTORE                                                                                                 \
		MRT_ROWSW_DECIDE(CNT_P, "", "", "")                                                                         \
		MRT_ROWSW_LEAF("s[60:61]", "s[62:63]", "", CNT_T, ANYA, ANYB, ANYDONE,                                      \
				MRT_ROWS_OWN_LEAF("s[60:61]"), MRT_ROWS_OWN_LEAF("s[62:63]"), OWN_RESTORE)                              \
		"L_pop_%=:\n"                                                                                               \
		MRT_ROWSW_POP("", "L_loop_%=")                                                                              \
		MRT_ROWSW_SLABS_OOL(BX, BY, BZ, OWN_KEEP)                                                                   \
		MRT_ROWSW_EXIT(MRT_ROWS_EXIT_WAIT, "s[60:61]", "s[62:63]")                                                  \
		: MRT_ROWSW_OUT                                                                                             \
		: MRT_ROWSW_IN_A(a), MRT_ROWSW_IN_B(b), [rows] "s"(rows), [qmask] "s"(qmask), [eps] "s"(eps), [vneg] "v"(vneg) \
		: MRT_ROWS_OWN_CLOBBER_##OWN_WHICH MRT_ROWS_CLOBBERS)
// the two copies: the general code, and the whole-tile fast path (entered with EXEC all ones)
#define MRT_ROWS_LOOPW_ARGS(...) MRT_ROWS_LOOPW_X(__VA_ARGS__)
#define MRT_ROWS_LOOPW(...) MRT_ROWS_LOOPW_ARGS(__VA_ARGS__, MRT_ROWS_OWN_ANYEXEC)
#define MRT_ROWS_LOOPW_WHOLE(...) MRT_ROWS_LOOPW_ARGS(__VA_ARGS__, MRT_ROWS_OWN_WHOLE)

// ---- the 128-ray walk with packet-level frustum culling ---------------------------------------------------------
// The ownership model (tools/sim_ownership.py, profiles/r03_ownership_sim_c3.json): of the (group, child box) slab
// tests a C3 packet executes, 46 % fail for all 64 rays of the group, and 87 % of those boxes lie wholly outside the
// pyramid the packet's 128 rays span: 40 % of the vector work of the walk buys nothing.  A box outside one side plane of
// the pyramid is one no ray of the packet reaches; both groups' tests of that child are skipped (masks zero).
// Round 2's form of the test (three per-lane loads per step, waited for on the spot) cost more than it saved: the
// kernel ran 8 % slower.  This form:
//   * ONE vector load per row brings the row's 16 dwords to lanes 0..15 of every 16-lane row of the wave (lane l reads
//     dword l & 15: the same 64-byte line for all four rows), so the four rows of the wave see the node's two child
//     boxes side by side: row r of the wave stands for side plane r of the pyramid;
//   * a lane multiplies its coordinate by its weight — the plane normal's component of that axis if the coordinate is
//     the one of the box's corner farthest along the normal, else 0 — and three DPP row_shr adds leave
//     dot(n', far corner) of the left child in lane 7 and of the right child in lane 15 of each row; one v_cmp against
//     the lane's constant cc = dot(n', apex) - eps (-inf in the other lanes) gives the cull bits: 6 vector
//     instructions per node step against 11 per (group, box) test skipped;
//   * the loads are issued ONE STEP AHEAD: when a node's row has arrived (scalar path) the vector copies of BOTH child
//     rows are requested, and waited for at the top of the next step, after this step's slab tests; a popped row's
//     copy is requested at the pop, beside its scalar fetch.  (The same loads pull both child rows towards the L2 for
//     the scalar fetch that follows: the far-child prefetch of MRT_ROWS_LOOPW is subsumed.)
// Soundness: see cull_setup().  v60 / v61: the vector copies of the left / right child row (or, after a pop, v60 of the
// popped row); s[66:67]: all ones when the current row's copy is the one in v61.  The weighted sum adds the products
// of eight lanes, five of them with weight 0: the row's ref / count dwords (integers < 2^26 or leaf-flagged: denormal
// bit patterns) times 0 are 0; a NaN or infinite coordinate (the padding box of a root leaf) makes the sum NaN and
// the compare false: not culled.
// One child box against one group (the arithmetic of MRT_ROWS_SLAB, one box at a time): TE = entry distance
// (v50 for the left child, v56 for the right one: what the near / far decision reads), MASK = lanes that hit
#define MRT_ROWS_SLAB1(P, RS, SIDE, TE, BX, BY, BZ, MASK)                                                             \
	"v_fma_f32 v51, " MRT_NEAR_##BX(RS, X, SIDE) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                      \
	"v_fma_f32 v52, " MRT_NEAR_##BY(RS, Y, SIDE) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                      \
	"v_fma_f32 v53, " MRT_NEAR_##BZ(RS, Z, SIDE) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                      \
	"v_fma_f32 v54, " MRT_FAR_##BX(RS, X, SIDE) ", " MRT_OP("ix", P) ", " MRT_OP("nrx", P) "\n"                       \
	"v_fma_f32 v55, " MRT_FAR_##BY(RS, Y, SIDE) ", " MRT_OP("iy", P) ", " MRT_OP("nry", P) "\n"                       \
	"v_fma_f32 v57, " MRT_FAR_##BZ(RS, Z, SIDE) ", " MRT_OP("iz", P) ", " MRT_OP("nrz", P) "\n"                       \
	"v_max_f32 v53, v53, " MRT_OP("tmin", P) "\n"                                                                   \
	"v_min_f32 v57, v57, " MRT_OP("lim", P) "\n"                                                                    \
	"v_max3_f32 " TE ", v51, v52, v53\n"                                                                            \
	"v_min3_f32 v54, v54, v55, v57\n"                                                                               \
	"v_cmp_le_f32_e64 " MASK ", " TE ", v54\n"

// one child (SIDE = L / R, TE its entry register, CULLBITS the bits of the cull word that speak for it): both groups
#define MRT_ROWSC_CHILD(SIDE, TE, CULLBITS, MA, MB, BX, BY, BZ)                                                       \
	"s_and_b32 s48, s44, " CULLBITS "\n"          /* some plane has the whole box outside? */                       \
	"s_cbranch_scc1 L_cull" #SIDE "_%=\n"                                                                           \
	"s_cmp_eq_u64 s[60:61], 0\n"                                                                                    \
	"s_cbranch_scc1 L_" #SIDE "A0_%=\n"                                                                             \
	MRT_ROWS_SLAB1("A", RA, SIDE, TE, BX, BY, BZ, MA)                                                               \
	"L_" #SIDE "A1_%=:\n"                                                                                           \
	"s_cmp_eq_u64 s[62:63], 0\n"                                                                                    \
	"s_cbranch_scc1 L_" #SIDE "B0_%=\n"                                                                             \
	MRT_ROWS_SLAB1("B", RA, SIDE, TE, BX, BY, BZ, MB)                                                               \
	"L_" #SIDE "B1_%=:\n"
#define MRT_ROWSC_CHILD_OOL(SIDE, MA, MB)                                                                             \
	"L_cull" #SIDE "_%=:\n"                                                                                         \
	MRT_ROWSC_CNT_CULL                                                                                              \
	"s_mov_b64 " MA ", 0\n"                                                                                         \
	"s_mov_b64 " MB ", 0\n"                                                                                         \
	"s_branch L_" #SIDE "B1_%=\n"                                                                                   \
	"L_" #SIDE "A0_%=:\n"                                                                                           \
	"s_mov_b64 " MA ", 0\n"                                                                                         \
	"s_branch L_" #SIDE "A1_%=\n"                                                                                   \
	"L_" #SIDE "B0_%=:\n"                                                                                           \
	"s_mov_b64 " MB ", 0\n"                                                                                         \
	"s_branch L_" #SIDE "B1_%=\n"
#define MRT_ROWSC_CNT_CULL ""

// request the vector copy of row REF (an SGPR) into VDST: lane l gets dword l & 15 of the row.  One vector instruction for
// the address (the scalar unit is the busier one in this loop: three scalar instructions per request made it the bound).
#define MRT_ROWSC_VLOAD(VDST, REF)                                                                                   \
	"v_lshl_add_u32 v62, " REF ", 6, %[cvo]\n"                                                                      \
	"global_load_dword " VDST ", v62, %[rows]\n"

// (No scalar-cache prefetch of the children here: the vector copies already pull both rows to the L2.)
// In: cur (group A's operand) = a row to visit, the groups' own masks, the lane's cull constants.  Out: cur = 0x7FFFFFFF.
// Stack entries as in MRT_ROWS_LOOPW.
#define MRT_ROWS_LOOPC(CNT_N, CNT_T, CNT_P, ANYA, ANYB, ANYDONE, BX, BY, BZ)                                          \
	asm volatile(                                                                                                   \
		"s_mov_b64 s[60:61], %[maskA]\n"                                                                            \
		"s_mov_b64 s[62:63], %[maskB]\n"                                                                            \
		MRT_ROWS_TOP_EMPTY \
		"L_vload_%=:\n"                           /* the current row's vector copy is not on its way yet */          \
		MRT_ROWSC_VLOAD("v60", "%[curA]")                                                                           \
		"s_mov_b64 s[66:67], 0\n"                                                                                   \
		"L_loop_%=:\n"                                                                                              \
		"s_lshl_b32 s52, %[curA], 6\n"                                                                              \
		"s_load_dwordx16 s[20:35], %[rows], s52\n"                                                                  \
		"s_waitcnt lgkmcnt(0)\n"                                                                                    \
		MRT_ROWS_HAVE \
		"s_bitcmp1_b32 %[curA], 31\n"                                                                               \
		"s_cbranch_scc1 L_tri_%=\n"                                                                                 \
		CNT_N                                                                                                       \
		"s_waitcnt vmcnt(0)\n"                    /* the row's vector copy (requested a step ago, or at the pop) */  \
		"v_cndmask_b32_e64 v58, v60, v61, s[66:67]\n"                                                               \
		"v_mul_f32 v58, v58, %[cw]\n"                                                                               \
		MRT_ROWSC_VLOAD("v60", RA_LREF)           /* both children's copies for the next step (also 2+ wait states */ \
		"v_add_f32_dpp v59, v58, v58 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n" /* before each DPP read) */ \
		MRT_ROWSC_VLOAD("v61", RA_RREF)                                                                             \
		"v_add_f32_dpp v58, v59, v59 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"                           \
		"s_nop 1\n"                                                                                                 \
		"v_add_f32_dpp v59, v58, v58 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"                           \
		"v_cmp_lt_f32_e64 s[44:45], v59, %[ccc]\n" /* bit 16 r + 7: the left box is outside plane r; 16 r + 15: the right one */ \
		"s_or_b32 s44, s44, s45\n"                                                                                  \
		MRT_ROWSC_CHILD(L, "v50", "0x00800080", "s[36:37]", "s[40:41]", BX, BY, BZ)                                 \
		MRT_ROWSC_CHILD(R, "v56", "0x80008000", "s[38:39]", "s[42:43]", BX, BY, BZ)                                 \
		/* the next row's vector copy: both children hit: the near one's, v60 (left) / v61; one child: its own */   \
		MRT_ROWSW_DECIDE(CNT_P, "s_cselect_b64 s[66:67], 0, -1\n", "s_mov_b64 s[66:67], 0\n", "s_mov_b64 s[66:67], -1\n") \
		MRT_ROWSW_LEAF("s[60:61]", "s[62:63]", "", CNT_T, ANYA, ANYB, ANYDONE, "", "", "")                          \
		"L_pop_%=:\n"                             /* the popped row's vector copy goes out beside its scalar fetch */ \
		MRT_ROWSW_POP(MRT_ROWSC_VLOAD("v60", RA_TOP) "s_mov_b64 s[66:67], 0\n", "L_vload_%=")                       \
		MRT_ROWSC_CHILD_OOL(L, "s[36:37]", "s[40:41]")                                                              \
		MRT_ROWSC_CHILD_OOL(R, "s[38:39]", "s[42:43]")                                                              \
		MRT_ROWSW_EXIT(MRT_ROWS_EXIT_WAIT, "s[60:61]", "s[62:63]")                                                  \
		: MRT_ROWSW_OUT                                                                                             \
		: MRT_ROWS_IN(A, a), MRT_ROWS_IN(B, b), [rows] "s"(rows), [qmask] "s"(qmask),                                \
		  [eps] "s"(eps), [vneg] "v"(vneg), [cw] "v"(cull.w), [ccc] "v"(cull.cc), [cvo] "v"(cull.voff)               \
		: MRT_ROWS_CLOBBERS, "v61", "v62")

// the lane's share of the packet's culling pyramid (see MRT_ROWS_LOOPC)
struct CullRegs {
	float w;          // weight of the lane's row dword: a component of the lane's plane normal, or 0
	float cc;         // lanes 7 and 15 of each 16-lane row: dot(n', apex) - eps; -inf elsewhere (and everywhere: never culls)
	uint32_t voff;    // byte offset of the lane's dword in a row
};

// counting builds of the one-packet loop also clock the row fetch: shader cycles from before the s_load to after
// its s_waitcnt (two s_memtime reads included), summed per wave in %[cntw].  At a pop the same pair brackets the popped row's
// fetch AND the stack entry's LDS reads issued under it (one wait for both): the longer of the two, which is the fetch.
#define MRT_ROWS_T_PRE "s_memtime s[64:65]\n s_waitcnt lgkmcnt(0)\n"
#define MRT_ROWS_T_POST "s_memtime s[66:67]\n s_waitcnt lgkmcnt(0)\n s_sub_u32 s64, s66, s64\n s_add_u32 %[cntw], %[cntw], s64\n"
#define MRT_ROWS_CNT_N "s_add_u32 %[cntn], %[cntn], 1\n"
// counting builds: the stack's high-water mark.  It follows the push's v_add_u32 of sp directly, and a VGPR written by the VALU needs one
// wait state before v_readfirstlane reads it (nothing pads the inside of an asm string): without the s_nop some waves read the
// pointer from before the push and the mark came out one entry low (tests/test_deep_trees_gpu.py)
#define MRT_ROWS_CNT_P "s_nop 0\n v_readfirstlane_b32 s52, %[spA]\n s_max_u32 %[cntp], %[cntp], s52\n"
#define MRT_ROWS_CNT_T "s_add_u32 %[cntt], %[cntt], 1\n"

// ---- the forms of a walk ----------------------------------------------------------------------------------------------------------
// A walk function holds 8 octants x (counting or not) x (any hit or nearest) asm blocks, of which a template instantiation keeps one.
// The eight octants: ROW(octant, sign bit of x, of y, of z)
#define MRT_OCTANTS(ROW) ROW(0, 0, 0, 0) ROW(1, 1, 0, 0) ROW(2, 0, 1, 0) ROW(3, 1, 1, 0) ROW(4, 0, 0, 1) ROW(5, 1, 0, 1) ROW(6, 0, 1, 1) ROW(7, 1, 1, 1)
// The four forms of octant O: LOOP(counting arguments, hit arguments, BX, BY, BZ) with COUNTING or PLAIN, ANY or NEAREST: the
// argument lists of that loop, as below
#define MRT_WALK_FORMS(LOOP, COUNTING, PLAIN, ANY, NEAREST, O, BX, BY, BZ)                                            \
	if (OCT == O) {                                                                                                 \
		if (COUNT) { if (ANY_HIT) LOOP(COUNTING, ANY, BX, BY, BZ); else LOOP(COUNTING, NEAREST, BX, BY, BZ); }      \
		else { if (ANY_HIT) LOOP(PLAIN, ANY, BX, BY, BZ); else LOOP(PLAIN, NEAREST, BX, BY, BZ); }                  \
	}
#define MRT_ROWS1_COUNTING MRT_ROWS_CNT_N, MRT_ROWS_CNT_T, MRT_ROWS_CNT_P, MRT_ROWS_T_PRE, MRT_ROWS_T_POST
#define MRT_ROWS1_PLAIN "", "", "", "", ""
#define MRT_ROWS1_ANY MRT_ROWS_ANYHIT("A", "4")
#define MRT_ROWS1_NEAREST MRT_ROWS_NEAREST("A")
#define MRT_ROWSW_COUNTING MRT_ROWS_CNT_N, MRT_ROWS_CNT_T, MRT_ROWS_CNT_P
#define MRT_ROWSW_PLAIN "", "", ""
#define MRT_ROWSW_ANY MRT_ROWSW_ANYHIT("A"), MRT_ROWSW_ANYHIT("B"), MRT_ROWSW_ANYDONE
#define MRT_ROWSW_NEAREST MRT_ROWS_NEAREST("A"), MRT_ROWS_NEAREST("B"), ""
// the eight cases of a switch on a wave-uniform octant: WALK<octant, ANY_HIT, COUNT>(arguments)
#define MRT_OCT_CASE(O, WALK, ...) case O: WALK<O, ANY_HIT, COUNT>(__VA_ARGS__); break;
#define MRT_OCT_SWITCH(OCT, WALK, ...)                                                                                \
	switch (OCT) { MRT_OCT_CASE(0, WALK, __VA_ARGS__) MRT_OCT_CASE(1, WALK, __VA_ARGS__) MRT_OCT_CASE(2, WALK, __VA_ARGS__) MRT_OCT_CASE(3, WALK, __VA_ARGS__) \
		MRT_OCT_CASE(4, WALK, __VA_ARGS__) MRT_OCT_CASE(5, WALK, __VA_ARGS__) MRT_OCT_CASE(6, WALK, __VA_ARGS__) MRT_OCT_CASE(7, WALK, __VA_ARGS__) }

// wave-uniform operands come back from an asm block as SGPRs; this tells the compiler they still are (MRT_UNIFORM: one counter)
#define MRT_UNIFORM(X) X = __builtin_amdgcn_readfirstlane(X)
__device__ __forceinline__ void rows_uniform(PacketRegs &s)
{
	s.cur = __builtin_amdgcn_readfirstlane(s.cur);
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)s.mask), hi = __builtin_amdgcn_readfirstlane((uint32_t)(s.mask >> 32));
	s.mask = ((unsigned long long)hi << 32) | lo;
}

template <int OCT, bool ANY_HIT, bool COUNT>
__device__ __forceinline__ void rows_walk_one(const float4 *rows, uint32_t qmask, PacketRegs &a, uint32_t &cnt_n, uint32_t &cnt_t, uint32_t &cnt_w, uint32_t &sp_max)
{
	const float eps = 1e-8f, vneg = -FLT_MAX;
	uint32_t ev = 0u;
	// (the counters go into the block as scalars: constants where nothing is counted, else told to be uniform as on the way out)
	if (!COUNT) { cnt_n = 0u; cnt_t = 0u; cnt_w = 0u; sp_max = 0u; }
	else { MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(cnt_w); MRT_UNIFORM(sp_max); }
#define MRT_ROW(O, BX, BY, BZ) MRT_WALK_FORMS(MRT_ROWS_LOOP1, MRT_ROWS1_COUNTING, MRT_ROWS1_PLAIN, MRT_ROWS1_ANY, MRT_ROWS1_NEAREST, O, BX, BY, BZ)
	MRT_OCTANTS(MRT_ROW)
#undef MRT_ROW
	rows_uniform(a);
	MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(cnt_w); MRT_UNIFORM(sp_max);
}

template <int OCT, bool ANY_HIT, bool COUNT>
__device__ __forceinline__ void rows_walk_wide(const float4 *rows, uint32_t qmask, PacketRegs &a, PacketRegs &b, uint32_t &cnt_n, uint32_t &cnt_t, uint32_t &sp_max)
{
	const float eps = 1e-8f, vneg = -FLT_MAX;
	if (!COUNT) { cnt_n = 0u; cnt_t = 0u; sp_max = 0u; }
	else { MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max); }
#define MRT_ROW(O, BX, BY, BZ) MRT_WALK_FORMS(MRT_ROWS_LOOPW, MRT_ROWSW_COUNTING, MRT_ROWSW_PLAIN, MRT_ROWSW_ANY, MRT_ROWSW_NEAREST, O, BX, BY, BZ)
	MRT_OCTANTS(MRT_ROW)
#undef MRT_ROW
	rows_uniform(a);
	MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max);
}

// the same walk for a wave that is entered with EXEC all ones (whole-tile pairs): it differs in the words of MRT_ROWS_OWNEXEC alone
template <int OCT, bool ANY_HIT, bool COUNT>
__device__ __forceinline__ void rows_walk_wide_whole(const float4 *rows, uint32_t qmask, PacketRegs &a, PacketRegs &b, uint32_t &cnt_n, uint32_t &cnt_t, uint32_t &sp_max)
{
#if MRT_ROWS_OWNEXEC
	const float eps = 1e-8f, vneg = -FLT_MAX;
	if (!COUNT) { cnt_n = 0u; cnt_t = 0u; sp_max = 0u; }
	else { MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max); }
#define MRT_ROW(O, BX, BY, BZ) MRT_WALK_FORMS(MRT_ROWS_LOOPW_WHOLE, MRT_ROWSW_COUNTING, MRT_ROWSW_PLAIN, MRT_ROWSW_ANY, MRT_ROWSW_NEAREST, O, BX, BY, BZ)
	MRT_OCTANTS(MRT_ROW)
#undef MRT_ROW
	rows_uniform(a);
	MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max);
#else
	rows_walk_wide<OCT, ANY_HIT, COUNT>(rows, qmask, a, b, cnt_n, cnt_t, sp_max);
#endif
}

template <int OCT, bool ANY_HIT, bool COUNT>
__device__ __forceinline__ void rows_walk_cull(const float4 *rows, uint32_t qmask, PacketRegs &a, PacketRegs &b, const CullRegs &cull, uint32_t &cnt_n, uint32_t &cnt_t, uint32_t &sp_max)
{
	const float eps = 1e-8f, vneg = -FLT_MAX;
	if (!COUNT) { cnt_n = 0u; cnt_t = 0u; sp_max = 0u; }
	else { MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max); }
#define MRT_ROW(O, BX, BY, BZ) MRT_WALK_FORMS(MRT_ROWS_LOOPC, MRT_ROWSW_COUNTING, MRT_ROWSW_PLAIN, MRT_ROWSW_ANY, MRT_ROWSW_NEAREST, O, BX, BY, BZ)
	MRT_OCTANTS(MRT_ROW)
#undef MRT_ROW
	rows_uniform(a);
	MRT_UNIFORM(cnt_n); MRT_UNIFORM(cnt_t); MRT_UNIFORM(sp_max);
}

// The packet's culling pyramid.  Culling is on only if every ray of the two tiles starts at one point (bit for bit),
// has t_min >= 0, and lies inside the four planes through the corner rays (lane 0 / 56 of tile A, lane 7 / 63 of tile B
// = the corners of the 16x8 block when B is A's right-hand neighbour) pushed outwards by 5e-5 rad: checked here for
// every lane, so any other arrangement (tiles on different image rows, rays that are not a pinhole grid, a partial
// tile without its corner lanes) simply does not cull.  Soundness: a box is skipped only if S < fl(dot(n', apex)) - eps,
// S = the rounded sum of the three rounded products n'_axis * corner_axis (relative error 2^-24 each, two real additions
// of at most 2^-24 of the partial sum each: |S - dot(n', corner)| <= 3 * 2^-24 |n'|_1 max|coordinate|), the right-hand
// side off by at most 4 * 2^-24 |n'|_1 |apex|_1, and eps = 8 * 2^-24 * |n'|_1 * (largest scene coordinate + |apex|_1),
// more than both together: so the true dot(n', corner - apex) is negative, the corner being the box's farthest point
// along n': no point of the box is on the inner side of that plane, and every ray point o + t d, t >= 0, is
// (dot(n', d) >= 1e-5 |d| was checked with the same roundings to spare).  The slab test such a ray makes against such a
// box fails by a margin (>= 1e-5 of the distance) three orders above its own rounding, so the skipped tests were
// all-false masks.
// Lane l: plane r = l >> 4 (top, right, bottom, left), row dword c = l & 15 = {lmin xyz, ref, lmax xyz, ref, rmin xyz, -,
// rmax xyz, -}.
__device__ __forceinline__ CullRegs cull_setup(const RayRegs &ra, const RayRegs &rb, bool valid_a, bool valid_b, unsigned long long part_a,
		unsigned long long part_b, float scene_abs_max, uint32_t lane)
{
	CullRegs c;
	c.w = 0.0f; c.cc = -__builtin_inff(); c.voff = (lane & 15u) * 4u;
	const bool corners = (part_a & 1ull) && (part_a >> 56 & 1ull) && (part_b >> 7 & 1ull) && (part_b >> 63 & 1ull);
	if (!corners) return c; // (wave-uniform)
#define MRT_RL(v, l) __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l))
	const float ox = MRT_RL(ra.ox, 0), oy = MRT_RL(ra.oy, 0), oz = MRT_RL(ra.oz, 0);
	const float tl[3] = { MRT_RL(ra.dx, 0), MRT_RL(ra.dy, 0), MRT_RL(ra.dz, 0) }, bl[3] = { MRT_RL(ra.dx, 56), MRT_RL(ra.dy, 56), MRT_RL(ra.dz, 56) };
	const float tr[3] = { MRT_RL(rb.dx, 7), MRT_RL(rb.dy, 7), MRT_RL(rb.dz, 7) }, br[3] = { MRT_RL(rb.dx, 63), MRT_RL(rb.dy, 63), MRT_RL(rb.dz, 63) };
	float cen[3] = { tl[0] + tr[0] + bl[0] + br[0], tl[1] + tr[1] + bl[1] + br[1], tl[2] + tr[2] + bl[2] + br[2] };
	const float cl = __builtin_sqrtf(cen[0] * cen[0] + cen[1] * cen[1] + cen[2] * cen[2]);
	if (!(cl > 0.0f)) return c;
	cen[0] /= cl; cen[1] /= cl; cen[2] /= cl;
	// the lane's plane: k = lane >> 4 -> (top, right, bottom, left) = cross of the two corner rays on that side
	const uint32_t k = lane >> 4;
	const float *pa = k == 0u ? tl : (k == 1u ? tr : (k == 2u ? br : bl)), *pb = k == 0u ? tr : (k == 1u ? br : (k == 2u ? bl : tl));
	float n[3] = { pa[1] * pb[2] - pa[2] * pb[1], pa[2] * pb[0] - pa[0] * pb[2], pa[0] * pb[1] - pa[1] * pb[0] };
	const float nl = __builtin_sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
	bool ok = nl > 0.0f;
	const float inv = ok ? 1.0f / nl : 0.0f;
	n[0] *= inv; n[1] *= inv; n[2] *= inv;
	if (n[0] * cen[0] + n[1] * cen[1] + n[2] * cen[2] < 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
	const float push = 5e-5f;
	n[0] += push * cen[0]; n[1] += push * cen[1]; n[2] += push * cen[2];
	// every lane checks its own two rays against ALL four planes (lanes 0, 16, 32, 48 hold one each)
	bool inside = true;
	for (int q = 0; q < 4; q++) {
		const float qx = MRT_RL(n[0], 16 * q), qy = MRT_RL(n[1], 16 * q), qz = MRT_RL(n[2], 16 * q);
		const float da = qx * ra.dx + qy * ra.dy + qz * ra.dz, la = __builtin_sqrtf(ra.dx * ra.dx + ra.dy * ra.dy + ra.dz * ra.dz);
		const float db = qx * rb.dx + qy * rb.dy + qz * rb.dz, lb = __builtin_sqrtf(rb.dx * rb.dx + rb.dy * rb.dy + rb.dz * rb.dz);
		if (valid_a && !(da >= 1e-5f * la)) inside = false;
		if (valid_b && !(db >= 1e-5f * lb)) inside = false;
	}
#undef MRT_RL
	if (valid_a && !(ra.ox == ox && ra.oy == oy && ra.oz == oz && ra.t_min >= 0.0f)) inside = false;
	if (valid_b && !(rb.ox == ox && rb.oy == oy && rb.oz == oz && rb.t_min >= 0.0f)) inside = false;
	ok = ok && __builtin_isfinite(n[0]) && __builtin_isfinite(n[1]) && __builtin_isfinite(n[2]);
	const bool planes_ok = (__ballot(ok) & 0x0001000100010001ull) == 0x0001000100010001ull;
	if (__ballot(!inside) != 0ull || !planes_ok) return c;
	const float n1 = __builtin_fabsf(n[0]) + __builtin_fabsf(n[1]) + __builtin_fabsf(n[2]);
	const float o1 = __builtin_fabsf(ox) + __builtin_fabsf(oy) + __builtin_fabsf(oz);
	const float err = 8.0f * 5.9604645e-8f * n1 * (scene_abs_max + o1);
	const float cc = (n[0] * ox + n[1] * oy + n[2] * oz) - err;
	if (__ballot(!__builtin_isfinite(cc)) != 0ull) return c;
	const uint32_t d = lane & 15u, axis = d & 3u;
	const bool is_max = (d >> 2 & 1u) != 0u;
	const float na = axis == 0u ? n[0] : (axis == 1u ? n[1] : n[2]);
	c.w = (axis < 3u && ((na >= 0.0f) == is_max)) ? na : 0.0f;   // the corner farthest along n': max where n' >= 0, else min
	c.cc = (d == 7u || d == 15u) ? cc : -__builtin_inff();
	return c;
}

__device__ __forceinline__ void rows_init(PacketRegs &s, const RayRegs &r, bool takes_part, uint32_t sp)
{
	s.ox = r.ox; s.oy = r.oy; s.oz = r.oz; s.dx = r.dx; s.dy = r.dy; s.dz = r.dz; s.tmin = r.t_min;
	s.ix = safe_inv(r.dx); s.iy = safe_inv(r.dy); s.iz = safe_inv(r.dz);
	s.nrx = -(r.ox * s.ix); s.nry = -(r.oy * s.iy); s.nrz = -(r.oz * s.iz);
	s.bt = r.t_max; s.bu = 0.0f; s.bv = 0.0f; s.bs = 0xFFFFFFFFu; s.bi = 0xFFFFFFFFu;
	s.lim = (!takes_part || r.t_min >= r.t_max) ? -FLT_MAX : r.t_max; // degenerate rays are misses, glsl:214-222
	s.sp = sp; s.cur = 0u; s.mask = 0ull;                              // the root is always a wide node
}

// wave-uniform octant of a packet's reciprocal directions over the lanes that take part (8 = mixed)
// (s.ix = safe_inv(r.dx), ..., as rows_init left them: the reciprocals are not worked out a second time)
__device__ __forceinline__ int rows_octant(const PacketRegs &s, bool part, unsigned long long &part_mask)
{
	part_mask = __ballot(part);
	const unsigned long long sx = __ballot(part && s.ix < 0.0f), sy = __ballot(part && s.iy < 0.0f), sz = __ballot(part && s.iz < 0.0f);
	const bool uniform = (sx == 0ull || sx == part_mask) && (sy == 0ull || sy == part_mask) && (sz == 0ull || sz == part_mask);
	return uniform ? ((sx ? 1 : 0) | (sy ? 2 : 0) | (sz ? 4 : 0)) : 8;
}

// the generic walk (mixed octants) reports a leaf-order slot: the row and the id the record is made from
__device__ __forceinline__ void rows_hit_of_slot(const float4 *rows, uint32_t n_nodes, uint32_t slot, PacketRegs &s)
{
	s.bs = 0xFFFFFFFFu;
	if (slot != 0xFFFFFFFFu) { s.bs = slot + n_nodes; s.bi = __float_as_uint(rows[(size_t)s.bs * 4u].w); }
}

// End of a ray in the row kernels: the record from what the walk holds.  The id is the one kept for the tie rule; layers and the
// normal are dwords 7 and 12..14 of the winning triangle's own row, a line the packet fetched moments ago (finish_ray gathers
// them from the hot and the cold array, which this kernel never touches otherwise).  Bool and token outputs need none of that.
template <bool STREAM>
__device__ __forceinline__ void finish_row_ray(const TraceParams &p, const float4 *rows, uint64_t ray_idx, const RayRegs &r,
		float best_t, float best_u, float best_v, uint32_t best_row, uint32_t best_id, uint32_t best_slot)
{
	int32_t prim = -1; float nx = 0.0f, ny = 0.0f, nz = 0.0f; uint32_t layers = 0u;
	if (best_row != 0xFFFFFFFFu) {
		if (p.out_fmt == OUT_BOOL8 || p.out_fmt == OUT_TOKEN4) prim = 0; // only "hit or not" (and the slot) is stored
		else {
			const float4 *row = rows + (size_t)best_row * 4u;
			prim = (int32_t)best_id;
			layers = __float_as_uint(reinterpret_cast<const float *>(row)[7]);
			const float4 nn = row[3];
			nx = nn.x; ny = nn.y; nz = nn.z;
		}
	}
	store_hit<STREAM>(p, ray_idx, r, best_t, prim, best_u, best_v, nx, ny, nz, layers, best_slot);
}

// ---- whole-tile pairs (lane_map.h fast_launch): 32-byte rays in, 32-byte records out, nothing to decide per launch -----------
template <bool STREAM>
__device__ __forceinline__ void load_ray32(const float4 *q, RayRegs &r)
{
	const float4 a = STREAM ? stream_load4(q) : q[0], b = STREAM ? stream_load4(q + 1) : q[1];
	r.ox = a.x; r.oy = a.y; r.oz = a.z; r.t_max = a.w;
	r.dx = b.x; r.dy = b.y; r.dz = b.z; r.t_min = b.w;
}
// the record of finish_row_ray + store_hit for OUT_HIT32
__device__ __forceinline__ void row_record32(const float4 *rows, float best_t, float best_u, float best_v, uint32_t best_row, uint32_t best_id, float4 &a, float4 &b)
{
	a.x = best_t; a.y = __int_as_float(-1); a.z = best_u; a.w = best_v;
	b.x = 0.0f; b.y = 0.0f; b.z = 0.0f; b.w = __uint_as_float(0u);
	if (best_row != 0xFFFFFFFFu) {
		const float4 *row = rows + (size_t)best_row * 4u;
		a.y = __uint_as_float(best_id);
		const float4 nn = row[3];
		b.x = nn.x; b.y = nn.y; b.z = nn.z;
		b.w = reinterpret_cast<const float *>(row)[7];
	}
}
struct RowsWave;
template <bool STREAM> __device__ __forceinline__ void rows_fast_records(const RowsWave &w, const PacketRegs &A, const PacketRegs &B);
// The kernel's arguments (its first one lies at the start of the argument block) through an address the compiler cannot tie to its
// first reading of them: what is read through it is read here and now.  Holds only while TraceParams is the kernel's FIRST argument
// (offset 0 of the argument block): trace_packet_rows_kernel takes it alone; an argument put in front of it breaks this.
__device__ __forceinline__ const __attribute__((address_space(4))) TraceParams *rows_args_again()
{
	const __attribute__((address_space(4))) TraceParams *q =
			(const __attribute__((address_space(4))) TraceParams *)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(q));
	return q;
}

// the wave-uniform words a wave keeps across its walks, for its records: whole-tile pairs the last two, else the others
struct RowsWave {
	uint32_t block_s, wave_s, tile_ax, tile_ay, tile_bx, tile_by, tile_code;
	uint32_t fast_ray, fast_w; // whole-tile pairs: the ray of tile A's first pixel, the row width
};
typedef __attribute__((address_space(3))) uint32_t *RowsStack; // a packet's stack in the LDS
// whole-tile pairs read the device's four grid words {width, rows, tiles_x, skip word} as one 16-byte load
static_assert((kAutoGridOff * sizeof(unsigned long long)) % 16u == 0u && (kDetectScratchOff - kAutoGridOff) * sizeof(unsigned long long) >= 16u,
		"the grid words of detect_grid_kernel: 16-byte aligned, four of them");
// whole-tile pairs: both records, from the two scalars, the lane, and the kernel's arguments read again
template <bool STREAM>
__device__ __forceinline__ void rows_fast_records(const RowsWave &w, const PacketRegs &A, const PacketRegs &B)
{
	const TraceParams &p2 = *(const TraceParams *)rows_args_again();
	const uint32_t lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
	float4 *out = reinterpret_cast<float4 *>(p2.hits) + (size_t)fast_lane_ray(w.fast_w, w.fast_ray, lane2) * 2u;
	const float4 *rows2 = reinterpret_cast<const float4 *>(p2.row_array);
	// both records first, then the four stores in a row: a store between the two rows' loads made the wave wait for its own stores
	// to come back (loads and stores share one counter), which a cast of short walks pays for with its bandwidth
	float4 aa, ab, ba, bb;
	row_record32(rows2, A.bt, A.bu, A.bv, A.bs, A.bi, aa, ab);
	row_record32(rows2, B.bt, B.bu, B.bv, B.bs, B.bi, ba, bb);
	if (STREAM) { stream_store4(out, aa); stream_store4(out + 1, ab); stream_store4(out + 16, ba); stream_store4(out + 17, bb); }
	else { out[0] = aa; out[1] = ab; out[16] = ba; out[17] = bb; }
}
// The second half of trace_packet_rows_kernel: the walks of the wave's packets and their records (defined below the kernel).
// FAST: whole-tile pairs, of which it does the paired walk alone; false = the wave's packets do not share an octant, nothing is done.
template <bool ANY_HIT, bool COUNT, int PACKETS, int WG, bool CULL, bool FAST>
__device__ __forceinline__ bool rows_walks_and_records(const TraceParams &p, RowsStack lds_a, RowsStack lds_b, uint32_t lane,
		RayRegs &ra, RayRegs &rb, bool valid_a, bool valid_b, const RowsWave &w);

#ifndef MRT_ROWS_WPE
#define MRT_ROWS_WPE 8
#endif
// PACKETS = 1: one packet per wave; 2: two (neighbouring tiles of the launch order).
// WG = threads per workgroup: 256 (four waves on neighbouring tiles share a CU and its scalar cache: C5 20.9 against
// 22.6 ms) or 64 (a wave slot is refilled as soon as ITS wave ends, not when a workgroup's worth of slots is free:
// C3 2.06 against 2.17 ms); api.hip picks by the size of the scene.
// CULL: paired packets walk with packet-level frustum culling (MRT_ROWS_LOOPC).
template <bool ANY_HIT, bool COUNT, int PACKETS, int WG, bool CULL = false>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(MRT_ROWS_WPE, 8))) void trace_packet_rows_kernel(const TraceParams p)
{
	// per wave and packet: 16-byte stack entries {ref, -, lane mask}; entry 0 holds the sentinel
	__shared__ __attribute__((aligned(16))) uint32_t wave_stack[WG / MRT_WAVE][PACKETS][(MRT_PACKET_STACK + 1) * 4];
	// Rays are read and records written once per launch: in the one-wave workgroups api.hip picks for scenes whose rows the caches can
	// hold (up to 256 MB) they stream past those rows (non-temporal: C3 1.89 -> 1.73 ms); beyond, the rows fit no cache either way (C5
	// measured the same with and without), and the 256-thread culling form spilled registers with the streaming loads.
	constexpr bool STREAM = WG == MRT_WAVE;
	uint32_t block = blockIdx.x;
	if (p.xcd_swizzle) {
		const uint32_t per = gridDim.x >> 3;
		if (block < (per << 3)) block = (block & 7u) * per + (block >> 3);
	}
	const uint32_t wave = threadIdx.x / MRT_WAVE, lane = threadIdx.x & (MRT_WAVE - 1);
	const uint32_t wave_s = __builtin_amdgcn_readfirstlane(wave), block_s = block; // (scalars: for the epilogue)
	// a lane without a ray in a packet walks along with an empty interval
	RayRegs ra = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}, rb = ra;
	bool valid_a = false, valid_b = false;
	uint32_t tile_ax = 0u, tile_ay = 0u, tile_bx = 0u, tile_by = 0u, tile_code = 0u;
	// Whole-tile pairs (lane_map.h fast_launch, asked by launch_trace; the grid's part here, where a width found on the device is
	// known): one division for the wave, two shifts and two adds for the lane, 32-bit up to the address, both rays always there.
	// The grid words and the skip word of a MAP_AUTO launch are one load.  Across the walk stay two scalars: the ray of tile A's
	// first pixel and the row width (the lane's index in a vector register of its own made the compiler spill to scratch).  The
	// paired walk and the records of such a wave are a copy of their own of the code below (rows_walks_and_records<.., true>): one
	// copy for both would make this path carry the other's words across the walk.
	if (PACKETS == 2 && !COUNT && p.rows_fast != kFastNo) {
		const uint32_t how = p.rows_fast;
		uint32_t gw = p.grid_w, n_rows = p.rows, tiles_x = p.tiles_x;
		if (how != kFastOwnGrid) {
			// (the four words detect_grid_kernel writes, 16-byte aligned: the static_assert on kAutoGridOff above the kernel)
			const uint4 found = *reinterpret_cast<const uint4 *>(p.auto_grid);
			if ((how == kFastAutoSkip) & (found.w == p.skip_when)) return;
			gw = found.x; n_rows = found.y; tiles_x = found.z;
		}
		if (fast_grid(gw, n_rows, tiles_x)) {
			uint32_t tx = 0u, ty = 0u;
			if (!fast_wave_tile(gw, n_rows, block_s * (WG / MRT_WAVE) + wave_s, tx, ty)) return; // past the last pair
			const RowsWave w = {0u, 0u, 0u, 0u, 0u, 0u, 0u, fast_tile_ray(gw, tx, ty), gw};
			const float4 *q = reinterpret_cast<const float4 *>(p.rays) + (size_t)fast_lane_ray(gw, w.fast_ray, lane) * 2u;
			load_ray32<STREAM>(q, ra);
			load_ray32<STREAM>(q + 16, rb); // (group B: the ray 8 on)
			if (rows_walks_and_records<ANY_HIT, COUNT, PACKETS, WG, CULL, true>(p, (RowsStack)wave_stack[wave_s][0], (RowsStack)wave_stack[wave_s][PACKETS - 1], lane, ra, rb, true, true, w))
				return;
			// the two tiles do not share an octant: on with the general code, as the two whole tiles of the general map they are
			valid_a = valid_b = true;
			tile_ax = tx; tile_ay = ty; tile_bx = tx + 1u; tile_by = ty; tile_code = kPieceTile | kPieceTile << 8 | 1u << 16;
		}
	}
	// Every other launch: the wave's tiles, once, on the scalar unit (lane_map.h): the second group's follows from the first's.  They
	// stay in scalar registers across the walk, for the epilogue: tile_a / tile_b = column | row of a tile, tile_code = the two pieces.
	// (The kernel's arguments are read again from here on: what this code needs of them -- most of them, some kept across the walks in
	// spill lanes -- is loaded here, not in the code every wave runs.)
	const TraceParams &pg = *(const TraceParams *)rows_args_again();
	if (tile_code == 0u) {
		if (skip_launch(pg)) return;
		const uint64_t group_a = ((uint64_t)block_s * (WG / MRT_WAVE) + wave_s) * PACKETS; // the wave's first group of 64 rays
		TileGrid tg;
		const bool tiled = tile_grid(pg, tg);
		WaveTile ta = {0u, 0u, kPieceNone}, tb = ta;
		if (tiled) {
			ta = wave_tile(tg, group_a);
			if (PACKETS == 2) tb = wave_tile_next(tg, ta, group_a);
		}
		tile_ax = __builtin_amdgcn_readfirstlane(ta.tx); tile_ay = __builtin_amdgcn_readfirstlane(ta.ty);
		tile_bx = __builtin_amdgcn_readfirstlane(tb.tx); tile_by = __builtin_amdgcn_readfirstlane(tb.ty);
		tile_code = __builtin_amdgcn_readfirstlane((ta.code & 0xFFu) | (tb.code & 0xFFu) << 8 | (tiled ? 1u << 16 : 0u));
		uint64_t idx = 0; uint32_t px = 0, py = 0;
		valid_a = tiled ? tile_lane(tg, ta, lane, idx, px, py) : linear_ray(pg, group_a, lane, idx, px, py);
		if (valid_a) load_ray<STREAM>(pg, idx, px, py, ra);
		if (PACKETS == 2) {
			valid_b = tiled ? tile_lane(tg, tb, lane, idx, px, py) : linear_ray(pg, group_a + 1u, lane, idx, px, py);
			if (valid_b) load_ray<STREAM>(pg, idx, px, py, rb);
		}
		if (__ballot(valid_a || valid_b) == 0ull) return; // nothing for this wave (otherwise every lane stays in)
		// the wave's start time waits in memory, not in registers (none to spare in the walk): in the cost array itself
		// (note_tile_start / note_tile_cost)
		if (pg.tile_cost != nullptr && lane == 0u) note_tile_start(pg, group_a << 6);
	}
	const RowsWave w = {block_s, wave_s, tile_ax, tile_ay, tile_bx, tile_by, tile_code, 0u, 0u};
	rows_walks_and_records<ANY_HIT, COUNT, PACKETS, WG, CULL, false>(pg, (RowsStack)wave_stack[wave][0], (RowsStack)wave_stack[wave][PACKETS - 1], lane, ra, rb, valid_a, valid_b, w);
}

template <bool ANY_HIT, bool COUNT, int PACKETS, int WG, bool CULL, bool FAST>
__device__ __forceinline__ bool rows_walks_and_records(const TraceParams &p, RowsStack lds_a, RowsStack lds_b, uint32_t lane,
		RayRegs &ra, RayRegs &rb, bool valid_a, bool valid_b, const RowsWave &w)
{
	constexpr bool STREAM = WG == MRT_WAVE;
	uint32_t *stack_a = (uint32_t *)lds_a, *stack_b = (uint32_t *)lds_b;
	const uint32_t block_s = w.block_s, wave_s = w.wave_s, tile_ax = w.tile_ax, tile_ay = w.tile_ay, tile_bx = w.tile_bx, tile_by = w.tile_by, tile_code = w.tile_code;
	const float4 *rows = reinterpret_cast<const float4 *>(p.row_array);
	// sentinels (volatile: the asm blocks have no "memory" clobber; they touch only read-only scene data and this stack)
	*(volatile __attribute__((address_space(3))) uint32_t *)&lds_a[0] = kSentinel;
	if (PACKETS == 2) *(volatile __attribute__((address_space(3))) uint32_t *)&lds_b[0] = kSentinel;
	PacketRegs A, B;
	rows_init(A, ra, valid_a, (uint32_t)(uintptr_t)(lds_a + 4));
	rows_init(B, rb, valid_b, (uint32_t)(uintptr_t)(lds_b + 4));

	unsigned long long part_a = 0ull, part_b = 0ull;
	const int oct_a = rows_octant(A, valid_a, part_a);
	const int oct_b = PACKETS == 2 ? rows_octant(B, valid_b, part_b) : 8;
	uint32_t cnt_n = 0u, cnt_t = 0u; // COUNT: node rows / triangle rows fetched by this wave
	uint32_t cnt_w = 0u;             // COUNT, one-packet loop: shader cycles between issuing a row fetch and having it
	uint32_t sp_wide = 0u, sp_one = 0u; // COUNT: highest stack pointers seen (LDS byte addresses) by the 128-ray / the one-packet walk
	// (the counting builds' start time waits in memory too: in the unused words of the stack's sentinel entry)
	if (COUNT) *(volatile __attribute__((address_space(3))) unsigned long long *)&lds_a[2] = __builtin_amdgcn_s_memtime();
	bool done_a = part_a == 0ull, done_b = part_b == 0ull;
	if (PACKETS == 2 && !done_a && !done_b && oct_a == oct_b && oct_a != 8) {
		// one walk for both groups: 32-byte stack entries over the wave's whole stack area, sentinel at its bottom;
		// at the root every lane that takes part owns the row
		*(volatile __attribute__((address_space(3))) uint32_t *)&lds_a[4] = kSentinel;
		A.sp += 16u; // (= stack base + 32)
		A.mask = part_a; B.mask = part_b;
		if (CULL) {
			const CullRegs cull = cull_setup(ra, rb, valid_a, valid_b, part_a, part_b, p.scene_abs_max, lane);
			MRT_OCT_SWITCH(oct_a, rows_walk_cull, rows, p.query_mask, A, B, cull, cnt_n, cnt_t, sp_wide)
		} else {
			if (FAST) { MRT_OCT_SWITCH(oct_a, rows_walk_wide_whole, rows, p.query_mask, A, B, cnt_n, cnt_t, sp_wide) }
			else { MRT_OCT_SWITCH(oct_a, rows_walk_wide, rows, p.query_mask, A, B, cnt_n, cnt_t, sp_wide) }
		}
		done_a = done_b = true;
		if (FAST) { rows_fast_records<STREAM>(w, A, B); return true; }
	}
	if (FAST) return false; // (tiles on an image axis, mixed directions in a tile: the general code below takes the wave on)
	// packets that could not be paired (different octants: tiles on an image axis; a single packet): one at a time
	if (!done_a && oct_a != 8) { MRT_OCT_SWITCH(oct_a, rows_walk_one, rows, p.query_mask, A, cnt_n, cnt_t, cnt_w, sp_one) done_a = true; }
	if (PACKETS == 2 && !done_b && oct_b != 8) { MRT_OCT_SWITCH(oct_b, rows_walk_one, rows, p.query_mask, B, cnt_n, cnt_t, cnt_w, sp_one) done_b = true; }
	const TraceParams &p2 = p;
	// best hit as the other kernels keep it: leaf-order slot = row - number of node rows
	uint32_t slot_a = A.bs == 0xFFFFFFFFu ? 0xFFFFFFFFu : A.bs - p2.n_nodes, slot_b = B.bs == 0xFFFFFFFFu ? 0xFFFFFFFFu : B.bs - p2.n_nodes;
	// mixed directions inside a packet: the generic compiler-scheduled walk over nodes + triangle arrays
	if (!done_a) {
		uint32_t nn = 0, nt = 0, nd = 0;
		A.bt = ra.t_max;
		packet_traverse<8, ANY_HIT, COUNT>(p2, ra, stack_a, A.bt, A.bu, A.bv, slot_a, nn, nt, nd, 0u, 0u, nullptr, !valid_a);
		if (COUNT) { cnt_n += __builtin_amdgcn_readfirstlane(nn); cnt_t += __builtin_amdgcn_readfirstlane(nt); }
		rows_hit_of_slot(rows, p2.n_nodes, slot_a, A);
	}
	if (PACKETS == 2 && !done_b) {
		uint32_t nn = 0, nt = 0, nd = 0;
		B.bt = rb.t_max;
		packet_traverse<8, ANY_HIT, COUNT>(p2, rb, stack_b, B.bt, B.bu, B.bv, slot_b, nn, nt, nd, 0u, 0u, nullptr, !valid_b);
		if (COUNT) { cnt_n += __builtin_amdgcn_readfirstlane(nn); cnt_t += __builtin_amdgcn_readfirstlane(nt); }
		rows_hit_of_slot(rows, p2.n_nodes, slot_b, B);
	}

	// The rays' indices again, from the wave's tiles (scalars) and the lane (the exec-mask count): no index, pixel or validity
	// flag stays live across the walk, where every vector register is spoken for (the compiler spilled 18 of them to scratch
	// around the assembly block: 0.3 GB of writes per C3 launch).  Only the lane's part of the map runs again.
	{
		const uint32_t lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
		const uint64_t h_a = ((uint64_t)block_s * (WG / MRT_WAVE) + wave_s) * PACKETS;
		const bool tiled2 = (tile_code >> 16 & 1u) != 0u;
		TileGrid tg2;
		(void)tile_grid(p2, tg2); // (of which the lane's part reads the clip rectangle and the tile's shape)
		const WaveTile ua = {tile_ax, tile_ay, tile_code & 0xFFu}, ub = {tile_bx, tile_by, tile_code >> 8 & 0xFFu};
		uint64_t idx2 = 0; uint32_t px2 = 0, py2 = 0;
		if (tiled2 ? tile_lane(tg2, ua, lane2, idx2, px2, py2) : linear_ray(p2, h_a, lane2, idx2, px2, py2))
			finish_row_ray<STREAM>(p2, rows, idx2, ra, A.bt, A.bu, A.bv, A.bs, A.bi, slot_a);
		if (PACKETS == 2 && (tiled2 ? tile_lane(tg2, ub, lane2, idx2, px2, py2) : linear_ray(p2, h_a + 1u, lane2, idx2, px2, py2)))
			finish_row_ray<STREAM>(p2, rows, idx2, rb, B.bt, B.bu, B.bv, B.bs, B.bi, slot_b);
		if (p2.tile_cost != nullptr && lane2 == 0u) note_tile_cost(p2, h_a << 6);
	}
	const unsigned long long t_start = COUNT ? *(volatile __attribute__((address_space(3))) unsigned long long *)&lds_a[2] : 0ull;
	if (COUNT && lane == 0u && (p2.count_mode != 2u || (blockIdx.x & 15u) == 0u)) { // the wave's clock: cycles in the row-fetch waits of the one-packet loop, cycles in all
		atomicAdd(&p2.counters[kCntFetchWaitCycles], (unsigned long long)cnt_w);
		atomicAdd(&p2.counters[kCntWaveCycles], __builtin_amdgcn_s_memtime() - t_start);
		atomicAdd(&p2.counters[kCntWaves], 1ull);
	}
	if (COUNT && p2.count_mode != 2u) { // the stack's high-water mark, in entries (the bound is the uploaded BVH's depth, <= 64: api.hip)
		const uint32_t base = (uint32_t)(uintptr_t)lds_a;
		const uint32_t e_wide = sp_wide > base ? (sp_wide - base) / 32u : 0u, e_one = sp_one > base ? ((sp_one - base) % 1040u) / 16u : 0u;
		atomicMax(&p2.counters[kCntMaxStack], (unsigned long long)(e_wide > e_one ? e_wide : e_one));
	}
	if (COUNT && p2.count_mode != 2u) { // (count_visits = 2: the clock only, sampled, so that the counting itself does not load the memory system)
		// per-ray words: every step of the wave is charged to every ray of the wave (both packets): an upper bound
		// per packet; the fetch words (kCntWaveNodeFetch / kCntWaveTriFetch) are exact
		if (valid_a) packet_count(p2, cnt_n, cnt_t, 0u, slot_a != 0xFFFFFFFFu, part_a | part_b);
		if (PACKETS == 2 && valid_b) { atomicAdd(&p2.counters[kCntRays], 1ull); if (slot_b != 0xFFFFFFFFu) atomicAdd(&p2.counters[kCntHits], 1ull); }
	}
	return true;
}
