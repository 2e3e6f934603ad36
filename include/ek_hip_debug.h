/*
 * ek_hip_debug.h -- tuning, profiling and test hooks of libek_hip.so.  NOT part of the drop-in
 * boundary (include/ek_hip.h): nothing a host of the reference's shape needs is declared here, and
 * these entries may change between rounds.  Used by bench.py (roofline instrumentation), tools/ and
 * the GPU test-suite (stage-level checks of the two-stage tridiagonalisation).
 */
#ifndef EK_HIP_DEBUG_H
#define EK_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Instrumentation for the roofline line of bench.py: enable = k > 0 brackets the launch of the
 * HBM-bound symv kernel of every k-th Householder column (one-stage path; k = 1: every launch; a
 * uniform sample over the trailing orders otherwise) by HIP events on its own stream; 0 switches it
 * off.  _get returns the accumulated device seconds, the number of timed launches and their
 * algorithmic bytes (8 B x lower triangle of the active matrix per launch). */
int ek_hip_profile_symv(int enable);
int ek_hip_profile_symv_get(double *seconds, long long *launches, double *algorithmic_bytes);

/* The same for the kernels of the two-stage path: seconds[i], launches[i] with i = 0 q2_apply_kernel
 * (application of the bulge-chasing reflectors, the largest kernel of a full-spectrum solve),
 * 1 chase_kernel, 2 symm_lower_kernel (every 8th panel), 3 unused. */
int ek_hip_profile_kernels(int enable);
int ek_hip_profile_kernels_get(double *seconds /* 4 */, long long *launches /* 4 */);

/* One-stage tridiagonalisation: tridiagonalise a device-generated synthetic matrix (order n, leading
 * dimension ld >= n rounded up to 128) `reps` times; *seconds = stage time per repetition. */
int ek_hip_debug_sytrd(int n, int ld, int reps, double *seconds);
unsigned long long ek_hip_debug_sytrd_work_bytes(int n);
int ek_hip_debug_sytrd_at(int n, int max_cols, int reps, double *dA, void *work, double *vecs, double *seconds);
int ek_hip_debug_gemm_at(int transa, int transb, int m, int n, int k, const double *dA, int lda, const double *dB,
                         int ldb, double beta, double *dC, int ldc, int lower_only, int reps, double *seconds);
/* Test hooks of the GEMM under every O(n^3) stage (ek_gemm.hip), at the level of its descriptor.
 *   _gemm_desc : ONE product C <- alpha op(A) op(B) + beta C, batched over `batch` entries, on the caller's DEVICE arrays at
 *            the caller's addresses, with every field of the descriptor: element strides between the entries, lower_only
 *            (tiles strictly above the diagonal are not referenced), staged_rank_k, small_tiles (lower_only on the 64-tiling)
 *            and even_offs.  offs (3 * batch: element offsets {A, B, C} of every entry, added to the strides) and dims
 *            (3 * batch: {M, N, K} of every entry, at most the m, n, k given) are optional HOST arrays the hook puts into
 *            device memory for the call.  Synchronises.  Returns 0, -k for an illegal k-th argument (also: an offset below
 *            zero -22, even_offs with an odd offset of A or B -21, an entry of dims outside 0 .. m, n, k -23) -- decided
 *            before any device work -- or <= -1000.
 *            variant[0..7] = what was launched: [0] the kernel (0 gemm_small_kernel, 1 gemm_kernel: 4 waves, 2 gemm_kernel_w8:
 *            8 waves, 3 gemm_rankk_kernel, -1 none: an empty product), [1] 1 the VEC instantiation / 0 the scalar one (rank-k:
 *            what the kernel's own test finds for one product without tables), [2] lower_only as launched (0; 1 the whole grid,
 *            tiles above the diagonal leave; 2 the compact grid), [3] the tile (64 or 128), [4] [5] tiles along M and N,
 *            [6] [7] the grid.
 *   _gemm_plan : the same decision alone, with the same arguments and the same -k (host arithmetic, no GPU: nothing is
 *            dereferenced but offs and dims).
 *   _gemm_compact_map : the compact grid's map workgroup -> tile for the workgroups first .. first + count - 1 of a
 *            tiles_m x tiles_n tiling (tiles_n <= tiles_m): tm[i], tn[i] and valid[i] (may be NULL; 0: the workgroup has no
 *            tile).  The kernels' own function compiled for the host, no GPU.  Returns the number of valid ones or -k. */
int ek_hip_debug_gemm_desc(int transa, int transb, int m, int n, int k, double alpha, double beta, const double *dA, int lda,
                           long long strideA, const double *dB, int ldb, long long strideB, double *dC, int ldc,
                           long long strideC, int batch, int lower_only, int staged_rank_k, int small_tiles, int even_offs,
                           const long long *offs, const int *dims, int *variant /* 8 */);
int ek_hip_debug_gemm_plan(int transa, int transb, int m, int n, int k, double alpha, double beta, const double *dA, int lda,
                           long long strideA, const double *dB, int ldb, long long strideB, double *dC, int ldc,
                           long long strideC, int batch, int lower_only, int staged_rank_k, int small_tiles, int even_offs,
                           const long long *offs, const int *dims, int *variant /* 8 */);
int ek_hip_debug_gemm_compact_map(int tiles_m, int tiles_n, long long first, int count, int *tm, int *tn, int *valid);
int ek_hip_debug_sytrd_split(void *alt, int mask);  /* placement experiments: sub-buffers of the scratch from alt */
int ek_hip_debug_set_sytrd_maxcols(int max_cols);   /* the hooks stop after max_cols columns (-1: all) */
int ek_hip_debug_sytrd_team(int n, int nteam, int reps, double *seconds);
int ek_hip_debug_reduce_team(int n, int nteam, int reps, double *seconds /* [2]: potrf, sygst */);

/* Two-stage tridiagonalisation, piece by piece on host arrays.
 *   _sy2sb : A (n x n, lda, symmetric, lower referenced) -> band (half bandwidth 64) left in the lower
 *            band of A, explicit reflectors V (n x n, ldv: column j = v_j, unit entry at row j + 64),
 *            tau (n); *flag: low byte 0 (a panel CholeskyQR2 cannot factor -- rank deficient, cond > 1e7 -- is factored
 *            by Householder reflections inside the stage), bits 8.. = the number of panels that took that rescue.
 *   _sb2st : the lower band of A -> d (n), e (n-1) by bulge chasing; Z (n x ncols, ldz; may be NULL
 *            with ncols = 0) <- Q2 Z; *flag bit 2 = the persistent kernel was abandoned.
 *   _two_stage_timing : seconds[0..3] = dense->band, band->tridiagonal, Q2 applied to ncols columns,
 *            Q1 applied, on a device-generated synthetic matrix.
 *   _set_two_stage : order from which the whole-path calls use two stages (-1 default, 0 never). */
int ek_hip_debug_sy2sb(int n, double *A, int lda, double *V, int ldv, double *tau, int *flag);
int ek_hip_debug_sb2st(int n, const double *A, int lda, double *d, double *e, double *Z, int ldz, int ncols, int *flag);
int ek_hip_debug_two_stage_timing(int n, int ncols, int reps, double *seconds, int *flag);
int ek_hip_debug_set_two_stage(int min_order);
/*   _sy2sb_stage : _sy2sb for the stage tests.  poison != 0: the stage's own workspace is filled with the NaN
 *            0x7FF8DEADBEEF1234 before the stage, so that whatever the stage reads of it before writing it shows in the
 *            output.  All of A, V, tau and flag are required.  Returns 0, -k for an illegal k-th argument (before any
 *            device work), or <= -1000.
 *   _set_sy2sb_flow : the rows of a trailing matrix from which the panels of _sy2sb go in pairs (pair_min) and from which
 *            the next panel is factored on the second stream beside the update (lookahead_min), on one GPU: each < 0 as
 *            its switch says (EK_SY2SB_PAIR_MIN, EK_SY2SB_LOOKAHEAD_MIN; the default), 0 never, > 0 that many rows.  Holds
 *            for every later call of the process, whole-path solves included, until it is set back to (-1, -1).
 *            Returns 0. */
int ek_hip_debug_sy2sb_stage(int n, double *A, int lda, double *V, int ldv, double *tau, int poison, int *flag);
int ek_hip_debug_set_sy2sb_flow(int pair_min, int lookahead_min);
/*   _sb2st_stage : _sb2st with what the stage leaves behind, in either workspace form.  form 0: the layout of _sb2st;
 *            form 1: what a whole-path solve does (the band packed by the caller into the stage's workspace without
 *            records, the records of Q2 lent as a separate array).  chase_mode 0: default, 1: sweeps through memory, 2:
 *            positions in registers.  Optional outputs (NULL: not wanted): V2 (n x n, ldv2; reflector (s, k) in rows
 *            s+1+64k .. min(s+64(k+1), n-1) of column s), tau2 ((kmax+1) x max(n-2, 1), ldtau; entry [k + s ldtau], kmax =
 *            (n-3)/64 + 1), *ran = which chase kernel ran (0: none, n < 3; 1: the sweep kernel alone; 2: the position
 *            kernel to the end; 3: it gave up and the sweep kernel redid the stage).  Z: any ncols >= 0, also above n.
 *            Returns 0, -k for an illegal k-th argument (before any device work), or <= -1000. */
int ek_hip_debug_sb2st_stage(int n, const double *A, int lda, int form, int chase_mode, double *d, double *e, double *V2,
                             int ldv2, double *tau2, int ldtau, double *Z, int ldz, int ncols, int *ran, int *flag);
/*   _sy2sb_team : the first stage over a 1 x P team (128-wide column strips, strip S on rank S mod P; per panel one
 *            broadcast of [V | T | tau] and one all-reduce of Y): nteam >= 1 rehearses the whole team inside this
 *            process (every member with its own copy of A -- NaN outside its strips when EK_HIP_TEAM_POISON=1), nteam = 0
 *            makes this process one rank of the attached communicator.  Out: the gathered band in the lower band of A
 *            (zero elsewhere), V and tau of member 0; *mismatch = entries in which the members' bands, V or tau differ. */
int ek_hip_debug_sy2sb_team(int n, double *A, int lda, double *V, int ldv, double *tau, int nteam, int *flag,
                            long long *mismatch);
int ek_hip_debug_sy2sb_team_timing(int n, int nteam, int reps, double *seconds);   /* device-generated matrix; whole team */
/* the same with the look-ahead threshold of the team form set (0: none, -1: default) and, optionally, HIP-event sums of
   the panel chains and of the "rest of the update" sections: parts[0..3] = stage, chains, rest-updates, and
   first chain + sum over panels of max(chain p + 1, update p / P) (seconds; meaningful with lookahead_min = 0) */
int ek_hip_debug_sy2sb_team_profile(int n, int nteam, int reps, int lookahead_min, double *seconds, double *parts);

/* Counters of this process's last whole-path solve: out[0] = flops the merge products of the divide & conquer
 * executed (2 M N K over both GEMMs of every merge, with the dimensions deflation and the column selection left
 * on the device: what bench.py prices that stage with, the nominal 4 n^3 / 3 being an upper bound), out[1] = 1
 * if the tridiagonalisation ran in two stages, out[2] = panels of the dense -> band stage that CholeskyQR2 could not
 * factor and the Householder rescue did, out[3] = 1 if the matrix was already a band of half width 64 on entry and
 * the dense -> band stage (and Q1) were skipped. */
int ek_hip_debug_last_solve_stats(double *out, int count);

/* workspace one whole-path call asks for (host arithmetic, no GPU): one GPU (nranks <= 1) or rank 0 of a 1 x nranks team;
   parts[0..5] (optional): one padded matrix, the persistent operators (L, Q1's reflectors), the eigenvector columns,
   X0 (the matrix, then the bulge chasing's reflectors), X1 (scratch of the reduction -> D&C bases -> Q2's records -> Q1's
   scratch), the rest.  ek_solve.hip plan_path. */
unsigned long long ek_hip_debug_workspace_bytes(int problem, int n, int n_vec, int nranks, unsigned long long *parts);

/* workspace one eigenvalues-only call (ek_hip_eigenvalues*) asks for (host arithmetic, no GPU): the same plan without
   the eigenvector array, the records of Q2, the scratch of Q1, of the D&C and of the back-transformation. */
unsigned long long ek_hip_debug_values_workspace_bytes(int problem, int n);
/* lanes per eigenvalue index of the bisection (ek_stebz.hip): 1, 2, 4, 8 or 16, each lane evaluating 2 points per pass
   (<= 0: the default, 4).  A tuning hook: the grid of the bisection, hence the last bits of the values, depends on it. */
int ek_hip_debug_set_stebz(int lanes);
/* workspace one window call (ek_hip_eigenpairs*) with m pairs asks for (host arithmetic, no GPU): jobz 0 the
   eigenvalues-only plan; range 0 with vectors the plan of n_vec = m; range 1 with vectors the full plan, grown where the
   window's compact D&C or back-transformation scratch could need more (m is then not referenced).  0: bad arguments. */
unsigned long long ek_hip_debug_window_workspace_bytes(int problem, int n, int jobz, int range, int m);
/* workspace one ek_hip_sygvx* call asks for (host arithmetic, no GPU): ek_hip_debug_window_workspace_bytes(1, n, jobz,
   range, m) for every itype 1..3 (types 2 and 3 keep type 1's plan).  0: bad arguments. */
unsigned long long ek_hip_debug_sygvx_workspace_bytes(int itype, int n, int jobz, int range, int m);
/* workspace one ek_hip_check_sparse_device call asks for (host arithmetic, no GPU), with a256(x) = x rounded up to a
   multiple of 256 bytes, csr(nnz) = a256(8 (n + 1)) + a256(8 nnz) + a256(16 nnz) (two entries per triplet, 4 + 8 bytes),
   n_orth = index2 - index1 + 1 (0 when index2 < index1), U = n_check for problem 0 and max(n_check, index2 if n_orth,
   n_ipr) for problem 1, ldt = U rounded up to 64 (at least 64), chunks = ceil(n / max(8, ceil(n / 128))):
     csr(nnzA) [+ csr(nnzB)] + a256(8 ldt n if U) [+ a256(8 ldt n if U) + a256(8 n U)] + a256(8 n_orth^2)
     + a256(8 chunks ldt if U) + a256(8 (max(n_check, n_orth) + 520)) + a256(8 (n_ipr + 8))
   with the bracketed terms for problem 1 only: Z^T, (B Z)^T, B Z, G, the chunks' partial sums, vectors, outputs.  No term
   is an n x n image of A or B.  0: bad arguments, n = 0, or nothing to do. */
unsigned long long ek_hip_debug_sparse_check_workspace_bytes(int problem, int n, long long nnzA, long long nnzB,
                                                             int n_check, int index1, int index2, int n_ipr);
/* the canonical form the sparse entries work on (host arithmetic, no GPU): the CSR of the mirrored symmetric matrix of a
   1-based triplet list -- rowptr (n + 1), col (0-based, ascending inside a row) and csr_val, the latter two with room for
   2 nnz entries.  Of the entries naming one unordered pair {i, j} the last of the list survives.  Returns the number of
   CSR entries, or -k for argument k (-3 also for an index outside 1 .. n). */
long long ek_hip_debug_sparse_csr(int n, long long nnz, const int *suf, const double *val, long long *rowptr, int *col,
                                  double *csr_val);
/* ek_hip_*_vbatched* and ek_hip_*_xvbatched*: 3 (the default, also for any other value) launches every class on a stream
   of its own (with an order above EK_HIP_BATCH_NMAX present there are up to four classes), 1 launches the classes one
   behind the other on one stream.  A tuning hook: no result depends on it. */
int ek_hip_debug_vbatched_streams(int streams);
/* the last ek_hip_eigenpairs_vbatched* call that was given `seconds`: device time of the launch of the classes of 128,
   64 and 32 (events around each on its stream) and the problems each took; either pointer may be NULL */
int ek_hip_debug_vbatched_last(double *class_seconds, int *class_count);
/* the same with four entries each: the classes of 256 (orders above EK_HIP_BATCH_NMAX, all chunks), 128, 64 and 32 of the
   last ek_hip_*_vbatched* or ek_hip_*_xvbatched* call that was given `seconds` */
int ek_hip_debug_xvbatched_last(double *class_seconds, int *class_count);
/* ek_hip_eigenpairs_xbatched*, orders above EK_HIP_BATCH_NMAX: problems per launch (a batch runs in chunks of that many,
   each chunk reusing the same image slots).  0 (or less) restores the default of 1024; returns the previous value.  A
   tuning and test hook: no result depends on it. */
int ek_hip_debug_xbatched_chunk(int problems);
/* ek_hip_eigenpairs_ybatched* and ek_hip_sygv_ybatched*, orders above EK_HIP_XBATCH_NMAX: problems per launch (a batch runs
   in chunks of that many, each chunk reusing the same image slots).  0 (or less) restores the default of 256; returns the
   previous value.  A tuning and test hook: no result depends on it. */
int ek_hip_debug_ybatched_chunk(int problems);
/* ek_hip_eigenpairs_window_batched*: problems per launch (a batch runs in chunks of that many, each chunk reusing the same
   slots of the inverse iteration's LU workspace).  0 (or less) restores the default of 1024; returns the previous value.
   A tuning and test hook: no result depends on it. */
int ek_hip_debug_window_batched_chunk(int problems);
/* ek_hip_eigenpairs_window_xbatched*, orders above EK_HIP_BATCH_NMAX: problems per launch (a batch runs in chunks of that
   many, each chunk reusing the same image and LU slots).  0 (or less) restores the default of 1024; returns the previous
   value.  A tuning and test hook: no result depends on it. */
int ek_hip_debug_window_xbatched_chunk(int problems);
/* ek_hip_*_window_xvbatched*: bytes of LU workspace the slots of one launch may sum to, for every class (a launch still
   takes at least one problem).  0 (or less) restores the defaults (1 GiB above EK_HIP_BATCH_NMAX, 256 MiB shared by the
   classes present below it); returns the previous value.  A tuning and test hook: no result depends on it. */
long long ek_hip_debug_window_xvbatched_budget(long long bytes);
/* ek_hip_check_xbatched* and ek_hip_check_sygv_xbatched*, orders above EK_HIP_BATCH_NMAX: checked problems per launch (a batch
   runs in chunks of that many, each chunk reusing the same scratch for S = B Z; types 2 and 3: for the products, L and W).
   0 (or less) restores the default of 1024; returns the previous value.  A tuning and test hook: no result depends on it. */
int ek_hip_debug_check_xbatched_chunk(int problems);
/* the last ek_hip_check_*vbatched* or ek_hip_check_*xvbatched* call that was given `seconds`: device time of the classes of
   256 (orders above EK_HIP_BATCH_NMAX, all chunks), 128, 64 and 32 (events between them on the one stream) and the problems
   each took; either pointer may be NULL.  The shape of ek_hip_debug_xvbatched_last.  NOT fed by
   ek_hip_check_window_xvbatched* and ek_hip_check_sygv_window_xvbatched*: they have one kernel class for every order, whose
   time is their `seconds`; the chunk size above governs their launches too. */
int ek_hip_debug_check_xvbatched_last(double class_seconds[4], int class_count[4]);

/* Test hooks of the stage entries of the generalized path (ek_hip_sygst, ek_hip_sygst_ibtype, ek_hip_trtrs; ek_chol.hip).
 *   _stage_leaves256 : 0 (the default, also for any value but 1): the solves of ek_hip_sygst, of type 1 of
 *            ek_hip_sygst_ibtype and of ek_hip_trtrs go through the 128-block inverses alone.  1: for n >= 256 they form
 *            the explicit inverses of L's 256 x 256 diagonal blocks and register them for the call, exactly as the
 *            whole-path call does, so that every solve takes the 256-leaves the whole path takes; the call's workspace
 *            grows by that array and its scratch.  Returns the previous mode.
 *   _set_sygst_direct : the order at or below which the reduction of every type (sygst_rec, sygst2_rec) reduces a block
 *            directly instead of recursing; <= 0 restores the default of 4096, values below 256 are raised to 256.
 *            Returns the previous order.  It governs the whole-path calls too.
 *   _sygst_scratch : returns the doubles of scratch a reduction of order n is given (sygst_scratch_doubles) and, in
 *            need[0..1] (optional), what the recursion of type 1 and of types 2 / 3 takes from it at the direct order
 *            as it stands (host arithmetic, no GPU).
 * No result's contract depends on either hook; the last bits may. */
int ek_hip_debug_stage_leaves256(int mode);
int ek_hip_debug_set_sygst_direct(int order);
unsigned long long ek_hip_debug_sygst_scratch(int n, unsigned long long *need /* 2 */);

/* test aid: the next `times` bulge chasings of whole-path calls count as abandoned (exercises the repetition from the
   saved band and the -992 exit of ek_solve.hip) */
int ek_hip_debug_fail_next_chase(int times);

/* Rehearsal of the divide & conquer's team form on one GPU (ek_stedc.hip, StedcTeam): while nranks >= 2, a grid cell solved
   WITHOUT a communicator (ek_hip_solve_device_grid / ek_hip_solve_replicated) forms the heights below the top merge that a
   team of nranks shards by strips rank after rank in this process (no exchange; same bits as any other form).  levels:
   sharded heights (-1: the library's default for the order and team); profile != 0: HIP events around the call and every
   rank's sections.  ek_hip_debug_stedc_team(0, -1, 0) switches it off.
   _get: seconds[0] the D&C, [1] all ranks' sections, [2] the longest rank's section summed over the heights -- a rank of
   a real team computes for [0] - [1] + [2] seconds (the all-gathers are not in it: one GPU). */
int ek_hip_debug_stedc_team(int nranks, int levels, int profile);
int ek_hip_debug_stedc_team_get(double *seconds);

/* The divide & conquer stage (ek_stedc.hip) in every storage form, on host arrays.  d (n), e (n - 1) -> all n eigenvalues
   ascending in w and eigenvector columns in Z (ldz >= n):
     nsel < 0   the full form: n columns (what ek_hip_stedc runs; first, nb, npcol, mycol are not referenced);
     nsel >= 0  the columns of ranks first + ((l / nb) * npcol + mycol) * nb + l % nb, l = 0 .. nsel - 1 (0-based), in
                columns 0 .. nsel - 1 of Z: a window on a 1 x 1 grid (npcol = 1, nb >= n; first > 0 there only) or a grid
                cell's block-cyclic share (first = 0).  The stage's own array is shaped as the whole path shapes it: n x n,
                or n x nsel with the compact bases when n > 32 and nsel <= n - n / 2.
   merges (optional, 6 * merge_cap ints): one record {off, n1, n, k, nrot, k1} per merge of the tree in plan order, height
   by height, the top merge last -- k poles survived the deflation, nrot pairs were rotated, k1 of the survivors are
   non-zero in the top n1 rows only (-1 when nrot > 0: the stage keeps no count of them that tells a dense column from an
   odd one).  The top merge is the one whose record has off = 0 and n = n.  *info: the stage's info.
   Returns the number of merges of the tree (0 for n <= 32; the records are filled when merge_cap holds them, -13
   otherwise), or -k for an illegal k-th argument (-4 also: a selected rank beyond n - 1; -5 also: first > 0 on a grid)
   -- decided before any device work -- or <= -1000. */
int ek_hip_debug_stedc(int n, const double *d, const double *e, int nsel, int first, int nb, int npcol, int mycol,
                       double *w, double *Z, int ldz, int *merges, int merge_cap, int *info);
/* columns of the n-row array ek_hip_debug_stedc gives the stage for that selection (host arithmetic, no GPU): nsel
   (at least 1) where the stage keeps its bases compact, n otherwise (nsel < 0: the full form).  -1: bad arguments. */
int ek_hip_debug_stedc_zcols(int n, int nsel);

/* The back-transformation Z <- Q Z, Q = H(0) ... H(n-2) (ek_ormtr.hip), as the whole path reaches it, on host arrays.
   V (n x n, ldv): the EXPLICIT reflectors, column j = v_j, zero above its unit entry (row j + 1 after the one-stage
   tridiagonalisation, row j + 64 after the dense -> band stage; a column of zeros with tau = 0 is the identity); tau
   (n - 1); Z (n x ncols, ldz) <- Q Z.  The T factors are formed ONCE (ormtr_prepare), then applied (ormtr_apply) to column
   slabs of `slab` columns (<= 0: one call over all ncols), every call with ncols_global (<= 0: ncols), the width the
   slicing of the inner dimension follows: a slab, or a grid cell's columns, given the whole Z's width carry the bits of
   the one call over the whole Z.  The workspace is the whole path's: ormtr_prep_bytes(n) and, for the widest slab w,
   ormtr_work_bytes(n, w, ncols_global) - ormtr_prep_bytes(n).  Returns 0, -k for an illegal k-th argument -- decided
   before any device work -- or <= -1000. */
int ek_hip_debug_ormtr(int n, int ncols, const double *V, int ldv, const double *tau, double *Z, int ldz,
                       int ncols_global, int slab);

/* Team Cholesky (ek_chol.hip potrf_lower_dist): look-ahead 0 off / 1 on / -1 default; profile != 0: HIP events around every
   owner's chain and every rest-of-update section of the next rehearsals (meaningful with the look-ahead OFF).  _get (after the
   rehearsal): parts[0] all chains, [1] all update sections, [2] first chain + sum over the strips of max(next chain, update / nteam):
   what the two cost a rank of a real team with the look-ahead. */
int ek_hip_debug_potrf_team_profile(int lookahead, int profile);
int ek_hip_debug_potrf_team_profile_get(int nteam, double *parts);

/* what the staging pipeline of the last ek_hip_solve on host arrays did: out[0] bytes in, [1] span of the input transfers
   (s), [2] busy seconds of the input workers, [3..5] the same on the way out, [6] seconds the main thread waited for
   inputs, [7] for the drain at the end, [8] 100 x workers on the way in + workers on the way out, [9] 0 (round 4: directions through a pinned ring, removed), [10] seconds from the start of the pipeline to its end, [11] seconds before the first input transfer */
int ek_hip_debug_last_pipe_stats(double *out, int count);

#ifdef __cplusplus
}
#endif
#endif /* EK_HIP_DEBUG_H */
