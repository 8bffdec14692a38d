// Probe hooks of libctrlora_hip.so: A/B switches between schedules / launch forms that compute the SAME result.
// They are exported for tests/tools/attn_bench.py, the A/B environment switches of ctrlora_amd/hip.py and the GPU
// tests that cover every form that ships; they are deliberately NOT declared in include/ctrlora_hip.h (the drop-in
// boundary): nothing a caller of the library needs, no effect on the input contract of any entry point.
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
/* attention schedule: 0 = default; 1 = tile-synchronous kernels only; 11 = backward with s_setprio;
 * 13 / 14 = hybrid forward (fragment lookahead 3 / 2) also where the pre-scaled-Q forward (attention_fwd40.hip) would
 * apply.  Unknown codes: CL_EINVAL, nothing changes. */
int cl_debug_attention_variant(int variant);   /* also 21 = 0 with the dK/dV kernel at FOUR key fragments per wave (round 6 probe: slower) */
/* 1 (default) = the dQ kernel forms delta itself; 0 = separate attn_delta launch */
int cl_debug_attention_fuse_delta(int on);
/* Read-only: what the last attention entry point of this process launched (csrc/attention.h: AttnLaunchRec; host side only, no
 * GPU touched).  out[0..15] = kind (0 nothing: the call was refused, 1 forward, 2 backward), family (1 tile-synchronous
 * transpose-free, 2 image-prompt, 3 hybrid, 4 pre-scaled d_head-40 forward, 5 fold backward, 6 transposed, 7 causal), dtype, d_head,
 * 64-row fragments per workgroup of the forward / dQ / dK-dV kernel (0 = did not run), bits (1 TAIL, 2 TQ, 4 TK template
 * forms, 8 s_setprio form), hybrid lookahead, workgroup remap, separate delta launch, dK/dV kernel ran, workgroups of the
 * forward / dQ / dK-dV kernel, tile length along the looped dimension.  CL_EINVAL for a null pointer. */
int cl_debug_attention_last_launch(int* out16);
/* GroupNorm launch forms: three_pass = 1 forces partial -> finalize -> apply; one_pass = 0 disables the one-launch
 * register-resident form (defaults 0, 1) */
int cl_debug_groupnorm_form(int three_pass, int one_pass);
/* The one-launch form with one workgroup per (sample, group) (csrc/norm.hip gng_*; bf16 only): 0 = never, 1 (default) = where the
 * shape rule takes it, 2 = whenever the slab fits the register budget (tests at small shapes); 5 / 6 = 1 / 2 with workgroup ids
 * mapped to (sample, group) pairs in plain order (timing aid: does the XCD placement matter?).  Off in any mode while
 * cl_debug_groupnorm_form asks for three launches or turns the one-launch forms off.  The probe reports form 5 with NV = vectors
 * per lane and operand, vectors per pixel row, threads per workgroup, C / G, grid B * G.  Other codes: CL_EINVAL, nothing changes. */
int cl_debug_groupnorm_group(int mode);
/* Read-only: what the last normalisation entry point of this process launched (csrc/norm.h: NormLaunchRec; host side only, no
 * GPU touched).  out[0..11] = kind (0 nothing: the call was refused, 1 / 2 GroupNorm forward / backward, 3 / 4 LayerNorm forward /
 * backward), form (1 one launch, 2 two launches, 3 three launches, 4 cooperative, 5 one launch with one workgroup per (sample, group); LayerNorm backward: 2 = with the finishing
 * kernel), dtype, NV (16-byte vectors per lane kept in registers; 0 for the chunked GroupNorm forms), LPR of the one-launch
 * GroupNorm / PY of the chunked ones / rows per wave iteration of the LayerNorm backward, waves (one-launch GroupNorm) or threads
 * per workgroup, CB (one-launch GroupNorm) / VX (chunked) / D / 8 (LayerNorm), pixel chunks per sample, grid x, grid y,
 * column-sum path of the LayerNorm backward (0 none, 1 workspace + finishing kernel, 2 atomics), channel passes per lane.
 * The cooperative form fills kind and form only.  CL_EINVAL for a null pointer. */
int cl_debug_norm_last_launch(int* out12);
/* Read-only: what the last weight-gradient entry point of this process (cl_weight_grad_tn, cl_weight_grad_tn_group) launched
 * (csrc/gemm.h: WgradLaunchRec; host side only, no GPU touched).  out[0..31] = ran (0 nothing: the call was refused, failed or had
 * nothing to add), launches of the single-product / single-tap kernel, of the row-of-three kernel, of the slab-reduce kernel,
 * problems launched, group launches, LDS ring depth and rows of m per step of the last group, then for the first eight group
 * launches (row-of-three kernel?, its grid, the reduce kernel's grid or 0).  CL_EINVAL for a null pointer.
 * cl_debug_wgrad_last_problem(i, out): problem i of that call in launch order, out[0..11] = row-of-three kind?, 128 x 128 tiles,
 * 32-row steps per split, splits, byte offset of its slabs in the workspace (-1: none, accumulated directly), first workgroup,
 * first reduce workgroup, index of the group launch it went into, index of its descriptor in the caller's array, M, N, K.
 * CL_EINVAL past the end (the record holds the first 4096 problems) or for a null pointer. */
int cl_debug_wgrad_last_launch(int* out32);
int cl_debug_wgrad_last_problem(int i, long* out12);
/* Read-only: what the last elementwise / layout entry point of this process (every launcher of csrc/elementwise.hip) launched
 * (csrc/elementwise.h: EwLaunchRec; host side only, no GPU touched).  out[0..7] = entry point (EW_* of elementwise.h; 0 nothing:
 * the call was refused, failed or had nothing to launch), dtype (-1: the entry point takes none), grid x, y, z and threads per
 * workgroup of its main kernel, form, aux.  form / aux -- colsum: 1 = block partials through the workspace + finishing kernel,
 * 2 = fp32 atomics, aux = pixel chunks per sample; zero: bit 0 = head bytes, bit 1 = tail bytes, aux = 16-byte vectors;
 * vit_patch_rows: 1 = float2 (PAIR) loads; mse_loss: aux = workgroups; transpose: dtype is the OUTPUT's, form = the input's
 * dtype (CL_BF16 / CL_F32).  CL_EINVAL for a null pointer. */
int cl_debug_ew_last_launch(int* out8);
/* 1 = GroupNorms whose groups span >= 1024 pixels run as one cooperative launch (csrc/norm_coop.hip: pixel slabs in
 * registers, the workgroups of a sample meet at a counter); 0 (default: measured no faster, see norm_coop.hip) = the forms above only.  _timeouts: how many workgroups ever gave
 * up waiting at that counter (0 unless something is broken; a timed-out launch produced wrong numbers) */
int cl_debug_groupnorm_coop(int on);
int cl_debug_groupnorm_coop_timeouts(void);
/* Launch tags for the contraction kernels (profiling aid: which SHAPE is a gemm dispatch of a kernel trace?).  While on, every
 * cl_gemm product signature {dtype, mode, M, N, K1, K2, act, residual} gets a small integer tag in order of first appearance
 * (1 .. 255) and each kernel it launches gets `tag` extra workgroups that exit at once -- so a trace row's Grid_Size names the
 * signature: workgroups = real grid + tag (tools/prof_shapes.py decodes it from the table below).  Results are unchanged.
 * cl_debug_gemm_tag_get(i, out): out[0..11] = dtype, mode, M, N, K1, K2, act, has_residual, tag, real workgroups of the main
 * kernel, workgroup size, launches so far; returns CL_EINVAL past the end. */
int cl_debug_gemm_tag(int on);
/* 1 (default) = product signatures WITHOUT a launch-table entry take the x-stationary kernel (gemm_xs.hip) where the rule in
 * gemm.hip says so; 0 = only where a table entry names configuration 34 (CTRLORA_GEMM_XS=0 sets 0 and drops those entries too) */
int cl_debug_gemm_xs_rules(int on);
/* LDS ring depth of the weight-gradient kernel: 3 (default since round 5: three workgroups per CU), 4 or 6 */
int cl_debug_wgrad_ring(int slots);
int cl_debug_gemm_tag_count(void);
/* empties the launch-tag table (it holds 255 signatures: a process that tags several models in turn clears it between them) */
int cl_debug_gemm_tag_clear(void);
int cl_debug_gemm_tag_get(int i, long* out12);
/* Read-only: the row of launch configuration `cfg` in the table every choice and dispatch of cl_gemm reads (csrc/gemm.hip: kCfgs).
 * out[0..9] = id, family (0 gemm_kernel, 1 gemm_fl_kernel, 2 x-stationary, 3 loader / consumer), BM, BN, WGM, WGN (MFMA waves),
 * KSUB (family 0), ring slots R, PRIO (family 1), flags: 1 persistent, 2 carries the GEGLU value | gate wave pair, 4 the same in bf16
 * only, 8 falls back to configuration 1 unless K is whole 128-byte lines, 16 ... or the product is not linear, 32 ... or N % BN.
 * CL_EINVAL for an id that has no row.  Touches no GPU. */
int cl_debug_gemm_config(int cfg, int* out10);
#ifdef __cplusplus
}
#endif
