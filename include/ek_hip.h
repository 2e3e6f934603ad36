/*
 * ek_hip.h -- C-ABI of libek_hip.so: the MI355X (gfx950) implementation of EigenKernel's
 * `scalapack` / `general_scalapack` / `*_select` solver path.
 *
 * Drop-in boundary.  The reference selects a back-end by the `-s <name>` string in
 * eigen_solver (src/solver_main.f90:52-99); each arm has the shape
 *     solve_with_<x>(n, proc, matrix_A, eigenpairs, matrix_B)         (:65)
 *     <solver>(proc, desc_A, A_local, [n_vec,] eigenpairs)            (:58, :62)
 * A Fortran maintainer adds arms `hip`, `hip_select`, `general_hip`, `general_hip_select`
 * that forward to ek_hip_solve through ISO_C_BINDING (stub in INTEGRATION.md).
 *
 * Conventions shared by every entry point:
 *   - plain C types only; all arrays fp64 column-major ("Fortran order");
 *   - `desc` is the 9-int ScaLAPACK descriptor with the reference's field order
 *     (src/descriptor_parameters.f90:2-4): [dtype=1, ctxt, M, N, MB, NB, rsrc, csrc, lld];
 *   - local arrays are `lld x numroc(N, NB, mycol, 0, npcol)` (distribute_matrix.f90:128-138);
 *   - the caller owns every array; the library borrows pointers for the duration of the
 *     call only (solver_scalapack_all.f90 allocates/deallocates around each call);
 *   - return value is LAPACK `info`: 0 = success, -k = argument k invalid,
 *     >0 = numerical failure of the stage (the reference aborts on info != 0 after
 *     pdpotrf/pdsygst/pdtrtrs: generalized_to_standard.f90:25-30,38-41,105-108),
 *     <= -1000 = HIP runtime error (-1000 - hipError_t);
 *     ek_hip_solve*: -4 also when A contains NaN/Inf; 100000 + k = the tridiagonal eigensolver
 *     failed (k <= n: QL iteration of the leaf containing row k; k = n+1: non-finite eigenvalue);
 *     the values -990 .. -999 are NOT argument indices (no entry has that many arguments) but
 *     states of the device pipeline and of the team, decided jointly by all ranks of a grid:
 *       -992  a bounded wait inside a persistent kernel of the two-stage path ran out (the
 *             application of the bulge-chasing reflectors was abandoned; outputs undefined),
 *       -993  another rank of the team failed (workspace, staging): this rank's
 *             own step was fine, the call ended on all ranks together,
 *       -994  rank / grid-cell mismatch with the attached communicator,
 *       -995  no communicator attached,  -996  exchange (RCCL / host hook) failed,
 *       -997  RCCL not loadable,  -998  no all-gather hook registered,  -999  the hook failed;
 *     a host of the reference's shape must test these before reading info < 0 as "argument -info
 *     illegal" (XERBLA's meaning); INTEGRATION.md section 4 has the table;
 *   - SPMD: called once, collectively, by the single main thread of every rank
 *     (main.f90:100-104), one rank per GPU.  Grids larger than 1x1 need a way to exchange data:
 *     the RCCL communicator (ek_hip_comm_init), the host communicator (ek_hip_comm_attach_host)
 *     or at least the all-gather hook (ek_hip_set_allgatherv); without any, a call with
 *     nprow*npcol != 1 returns the negative index of the offending argument.
 *   - there is no CPU fallback anywhere behind this interface.
 */
#ifndef EK_HIP_H
#define EK_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define EK_HIP_N_STAGES 8
/* indices into stage_seconds[]; names are the reference's add_event names
 * (generalized_to_standard.f90:33,44,111; solver_scalapack_all.f90:66,93,104,122) */
#define EK_STAGE_POTRF   0  /* reduce_generalized:pdpotrf              */
#define EK_STAGE_SYGST   1  /* reduce_generalized:pdsygst              */
#define EK_STAGE_SYTRD   2  /* eigen_solver_scalapack_all:pdsytrd      */
#define EK_STAGE_GATHER  3  /* eigen_solver_scalapack_all:gather1      */
#define EK_STAGE_STEDC   4  /* eigen_solver_scalapack_all:pdstedc      */
#define EK_STAGE_ORMTR   5  /* eigen_solver_scalapack_all:pdormtr      */
#define EK_STAGE_TRTRS   6  /* recovery_generalized                    */
#define EK_STAGE_COPY    7  /* host<->device staging (not in the reference) */

/* Library / device management ---------------------------------------------------------- */
int ek_hip_version(void);                       /* 100*major + minor.  2: round 5 (version 1's
                                                 * ek_hip_comm_peer_enable / _disable are gone since
                                                 * round 4: INTEGRATION.md 5); 3: the eigenvalues-only
                                                 * entries ek_hip_eigenvalues* and ek_hip_stebz.  Still 3
                                                 * with the window entries ek_hip_eigenpairs* and
                                                 * ek_hip_stebz_range, and with ek_hip_sygvx*,
                                                 * ek_hip_sygst_ibtype and ek_hip_trmm, and with
                                                 * ek_hip_eigenpairs_batched*,
                                                 * ek_hip_eigenpairs_vbatched*, ek_hip_check_batched*
                                                 * and ek_hip_check_vbatched*, and with
                                                 * ek_hip_sygv_batched_device, ek_hip_sygv_batched,
                                                 * ek_hip_sygv_vbatched_device and
                                                 * ek_hip_sygv_vbatched, and with the triplet entries
                                                 * ek_hip_solve_sparse, ek_hip_check_sparse* and
                                                 * ek_hip_sparse_to_dense: their symbols are the signal */
int ek_hip_init(int device);                    /* bind this process (rank) to a GPU        */
int ek_hip_finalize(void);                      /* release cached workspaces / device images */
const char *ek_hip_stage_name(int stage);       /* reference event name of a stage index    */

/* Whole path -- replaces solve_with_general_scalapack (solver_scalapack_all.f90:127-168),
 * eigen_solver_scalapack_all (:19-124) and, with n_vec < n, the *_select arms
 * (solver_main.f90:59-75, solver_scalapack_select.f90:14-69).
 *   problem : 0 standard (A x = l x), 1 generalized (A x = l B x, B SPD)
 *   n_vec   : n for the full spectrum; < n only for the *_select arms
 *   A_loc   : in: symmetric, lower triangle referenced; out: Householder reflectors
 *             below the sub-diagonal (as PDSYTRD leaves it; from order 512 on, two-stage
 *             reduction: the band and the first stage's R factors -- INTEGRATION.md)
 *   B_loc   : in: SPD, lower; out: Cholesky factor L (needed by recovery); NULL if problem==0
 *             (uplo = 'L' as everywhere in the reference: the strictly upper triangles of A_loc
 *             and B_loc are never referenced and, on a 1 x 1 grid, never written -- the caller
 *             finds there what it left there, as after PDPOTRF / PDSYTRD; from order 2048 on only
 *             the lower triangles cross PCIe.  On larger grids the local block-cyclic pieces are
 *             written whole: the entries of a piece that lie strictly above the GLOBAL diagonal
 *             come back with UNSPECIFIED FINITE values (what the stages left in the library's
 *             work array), never NaN or Inf -- tests/test_gpu_path.py holds the library to that.)
 *   w       : out: n doubles, ascending, first n_vec valid (eigenpairs%blacs%values)
 *   Z_loc   : out: eigenvectors (eigenpairs%blacs%Vectors), N x N descriptor, same NB as A;
 *             B-orthonormal (generalized) / orthonormal (standard)
 *   stage_seconds : NULL or EK_HIP_N_STAGES doubles (device time of each stage)
 */
int ek_hip_solve(int problem, int n, int n_vec,
                 double *A_loc, const int desc_A[9],
                 double *B_loc, const int desc_B[9],
                 double *w,
                 double *Z_loc, const int desc_Z[9],
                 int nprow, int npcol, int myrow, int mycol,
                 double *stage_seconds, int n_stages);

/* Same computation on arrays that already live in device memory (HBM) of the bound GPU:
 * dA (lda), dB (ldb), dZ (ldz) column-major n x n, dw n doubles.  This is what bench.py
 * times.  Asynchronous errors are reported by the return value (the call synchronises).
 * IN PLACE: the call owns dA, dB and dZ for its duration.  Arrays that already have the
 * library's internal layout (n a multiple of 128, leading dimension n, 256-byte aligned base)
 * ARE its work arrays, any other is copied in and out -- either way, on return: dA = what the
 * tridiagonalisation leaves (lower triangle: reflectors / band and R factors), dB = L (lower
 * triangle), dZ = the eigenvectors; the strictly UPPER triangles of dA and dB hold scratch of
 * the stages (they are not referenced as inputs and not restored).  After an error return
 * (info != 0: a failing pivot, -4, -992 ...) dA, dB and dZ hold intermediate state -- as A and
 * B do after a failed PDPOTRF / PDSYGST: a caller that needs its inputs again keeps a copy.
 * (EK_HIP_ALIAS=0: always through internal copies; the inputs are then overwritten only by
 * the final copy-out.) */
int ek_hip_solve_device(int problem, int n, int n_vec,
                        double *dA, int lda, double *dB, int ldb,
                        double *dw, double *dZ, int ldz,
                        double *stage_seconds, int n_stages);

/* Eigenvalues only -- LAPACK DSYGVD / DSYEVD with JOBZ = 'N', DSYEVX with RANGE = 'I': the same reduction and
 * tridiagonalisation as ek_hip_solve, then bisection with Sturm counts on the GPU (ek_hip_stebz) in place of the
 * divide & conquer; no eigenvectors are formed, nothing is back-transformed or recovered, and the call reserves no
 * eigenvector or back-transformation workspace.  NOT COLLECTIVE: it computes on the bound GPU alone and uses no grid
 * and no communicator, even when one is attached.
 *   problem, A, B : as in ek_hip_solve (0 standard, 1 generalized with B SPD; lower triangles referenced)
 *   il, iu        : 1-based indices of the wanted eigenvalues in ascending order, 1 <= il <= iu <= n (n = 0: nothing)
 *   w             : out: iu - il + 1 doubles, ascending.  The value of an index is bit-identical whatever [il, iu]
 *                   is asked for; absolute accuracy about 2 eps max|lambda| of the tridiagonal stage (normwise, as
 *                   the divide & conquer's)
 *   stage_seconds : NULL or up to EK_HIP_N_STAGES doubles: the bisection in EK_STAGE_STEDC, EK_STAGE_ORMTR and
 *                   EK_STAGE_TRTRS are 0
 * info: -k for argument k; -5 also when A contains NaN/Inf; a B that is not SPD gives the positive info of
 * ek_hip_solve_device for that B; <= -1000 HIP runtime error; -992 as in ek_hip_solve. */
/* problem 0/1 as ek_hip_solve; w receives iu-il+1 doubles, ascending; 1 <= il <= iu <= n (n = 0: nothing)
 * in place, as ek_hip_solve_device: dA and dB (device, lda / ldb) come back as that call leaves them after the
 * tridiagonalisation (dA) and the Cholesky factorisation (dB); dw is device memory */
int ek_hip_eigenvalues_device(int problem, int n, int il, int iu, double *dA, int lda, double *dB, int ldb,
                              double *dw, double *stage_seconds, int n_stages);
/* host arrays A (lda), B (ldb), w; A and B are left untouched (the call works on device copies) */
int ek_hip_eigenvalues(int problem, int n, int il, int iu, const double *A, int lda, const double *B, int ldb,
                       double *w, double *stage_seconds, int n_stages);
/* The stage alone, host arrays: DSTEBZ('I', 'E') -- eigenvalues il..iu (1-based, ascending) of the symmetric
 * tridiagonal d(n), e(n-1) into w(iu-il+1), bit-identical per index whatever the range.  info -k for argument k
 * (-2 / -3 also for NaN / Inf in d / e). */
int ek_hip_stebz(int n, const double *d, const double *e, int il, int iu, double *w);

/* A window of eigenpairs -- LAPACK DSYEVX / DSYGVX, ScaLAPACK PDSYEVX with RANGE = 'I' or 'V': the same reduction and
 * tridiagonalisation as ek_hip_solve; then, for values only, the bisection of ek_hip_eigenvalues, and for values and
 * vectors the divide & conquer restricted to the window's eigenvectors (its top merge forms those columns alone), with
 * the back-transformation and the recovery on those m columns.  NOT COLLECTIVE, as ek_hip_eigenvalues.
 *   problem, A, B : as in ek_hip_solve (0 standard, 1 generalized with B SPD; lower triangles referenced)
 *   jobz          : 0 values only, 1 values and eigenvectors
 *   range         : 0 = 'I': indices il..iu (1-based, 1 <= il <= iu <= n; vl, vu not referenced)
 *                   1 = 'V': the eigenvalues in the half-open interval (vl, vu], vl < vu, -Inf / +Inf allowed (il, iu
 *                   not referenced); the bounds are counted on the tridiagonal (Sturm counts, as DSTEBZ), so a bound
 *                   within rounding of an eigenvalue may count it on either side
 *   m, ifirst     : out: the number of pairs and the global 1-based index of the first (m = 0 is success)
 *   w             : out: m eigenvalues, ascending; room for iu-il+1 ('I') or n ('V') doubles.  A value is
 *                   bit-identical to the one ek_hip_eigenvalues returns for its index when jobz = 0, and to the one
 *                   ek_hip_solve_device returns when jobz = 1.  The two may differ in the last bits.
 *   Z, ldz, zcap  : jobz = 1: n x zcap, ldz >= n; columns 0..m-1 receive the eigenvectors of indices ifirst..ifirst+m-1
 *                   (B-orthonormal for problem 1).  Not referenced when jobz = 0.  m > zcap: info -18 with *m set and
 *                   nothing written to w or Z ('I': before any device work; 'V': after the count)
 *   stage_seconds : NULL or up to EK_HIP_N_STAGES doubles: the count and the divide & conquer or the bisection in
 *                   EK_STAGE_STEDC
 * Workspace: values only, the eigenvalues-only plan; 'I' with vectors, the plan of ek_hip_solve_device with n_vec = m;
 * 'V' with vectors, the full plan (m is known only after the tridiagonalisation).
 * info: -k for argument k (checked before any device work; -9 also when A contains NaN/Inf); a B that is not SPD gives
 * the positive info of ek_hip_solve_device for that B; <= -1000 HIP runtime error; -992 as in ek_hip_solve.
 * The device form works in place as ek_hip_eigenvalues_device: dA and dB come back as after the tridiagonalisation
 * (dA) and the Cholesky factorisation (dB); dw and dZ are device memory. */
int ek_hip_eigenpairs_device(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu,
                             double *dA, int lda, double *dB, int ldb, int *m, int *ifirst,
                             double *dw, double *dZ, int ldz, int zcap, double *stage_seconds, int n_stages);
/* host arrays A (lda), B (ldb), w, Z (ldz); A and B are left untouched (the call works on device copies) */
int ek_hip_eigenpairs(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu,
                      const double *A, int lda, const double *B, int ldb, int *m, int *ifirst,
                      double *w, double *Z, int ldz, int zcap, double *stage_seconds, int n_stages);
/* The stage alone, host arrays: DSTEBZ('V', 'E') -- the eigenvalues of the symmetric tridiagonal d(n), e(n-1) in
 * (vl, vu]: *il = the 1-based index of the first, *m = their number, w (n doubles) the values, bit-identical to what
 * ek_hip_stebz returns for il..il+m-1.  info -k for argument k (-2 / -3 also for NaN / Inf in d / e). */
int ek_hip_stebz_range(int n, const double *d, const double *e, double vl, double vu, int *il, int *m, double *w);

/* DSYGVX / PDSYGVX: the three generalized problems, B SPD, lower triangles of A and B referenced --
 *   itype 1: A x = l B x   (C = L^-1 A L^-T, x = L^-T y; X^T B X = I)
 *   itype 2: A B x = l x   (C = L^T A L,     x = L^-T y; X^T B X = I)
 *   itype 3: B A x = l x   (C = L^T A L,     x = L y;    X^T B^-1 X = I)
 * with B = L L^T.  jobz, range, vl, vu, il, iu, m, ifirst, w, Z, ldz, zcap, stage_seconds: exactly as
 * ek_hip_eigenpairs* (argument k here is argument k there, with itype in the place of problem); types 2 and 3 report
 * their reduction in EK_STAGE_SYGST and their recovery in EK_STAGE_TRTRS.  NOT COLLECTIVE, one GPU.
 * info: -1 for itype outside 1..3, then as ek_hip_eigenpairs*: -9 also for NaN / Inf in A, the positive info of
 * ek_hip_solve_device for a B that is not SPD.  itype 1 returns w and Z bit-identical to ek_hip_eigenpairs*(problem 1);
 * types 2 and 3 return bit-identical eigenvalues for the same A and B.  The workspace is type 1's for every type. */
int ek_hip_sygvx_device(int itype, int jobz, int range, int n, double vl, double vu, int il, int iu,
                        double *dA, int lda, double *dB, int ldb, int *m, int *ifirst,
                        double *dw, double *dZ, int ldz, int zcap, double *stage_seconds, int n_stages);
/* host arrays A (lda), B (ldb), w, Z (ldz); A and B are left untouched (the call works on device copies) */
int ek_hip_sygvx(int itype, int jobz, int range, int n, double vl, double vu, int il, int iu,
                 const double *A, int lda, const double *B, int ldb, int *m, int *ifirst,
                 double *w, double *Z, int ldz, int zcap, double *stage_seconds, int n_stages);

/* Many small problems in one call -- what syevjBatched / sygvdBatched are to cuSOLVER / rocSOLVER users: `batch`
 * independent problems of one order n <= EK_HIP_BATCH_NMAX, strided in memory, solved by ONE kernel launch in which a
 * workgroup owns a problem from its first load to its last store and keeps the matrix in LDS (Cholesky, reduction to
 * standard form, Householder tridiagonalisation, implicit QL, back-transformation, recovery: no launch between them).
 * NOT COLLECTIVE: one GPU, no grid, no communicator; the call synchronises.
 *   problem, jobz : as in ek_hip_eigenpairs* (0 standard / 1 generalized with B SPD; 0 values / 1 values and vectors)
 *   n, batch      : 0 <= n <= EK_HIP_BATCH_NMAX, batch >= 0 (n = 0 or batch = 0: success, nothing referenced)
 *   A, lda, strideA : problem b's A is the column-major n x n array at A + b * strideA, lda >= n, strideA >= lda * n
 *                   (a stride of 0 is an argument error, not a broadcast); lower triangle referenced
 *   B, ldb, strideB : the same for B; not referenced (may be NULL) when problem = 0
 *   w             : out: batch x n doubles, problem b's eigenvalues ascending at w + b * n
 *   Z, ldz, strideZ : out (jobz = 1): problem b's eigenvectors at Z + b * strideZ, ldz >= n, strideZ >= ldz * n, column k
 *                   belonging to w[b * n + k]; orthonormal, B-orthonormal for problem 1.  Not referenced when jobz = 0
 *   info          : out: HOST array of batch ints, one per problem: 0 success; k > 0: B is not SPD (a NaN in B
 *                   included), k the 1-based failing pivot -- the value ek_hip_solve_device returns for that B;
 *                   -5: the lower triangle of that A holds NaN / Inf; 100000 + k: the QL iteration failed as in
 *                   ek_hip_solve (k = n + 1: the reduction left a non-finite tridiagonal, or an eigenvalue lies beyond
 *                   the range of a double: info = 0 always comes with finite w).  The w and Z slots of a
 *                   failed problem hold unspecified values; nothing outside its own slots is written and the other
 *                   problems of the batch are unaffected
 *   seconds       : NULL or one double: device time of the launch (events around it)
 * Return value: 0 when the arguments were legal and the launch ran (whatever info[] says); -k for argument k, decided
 * before any device work; <= -1000 HIP runtime error.
 * A problem's result does not depend on the batch around it: the same (A, B) gives bit-identical w and Z alone, at
 * any position of any batch, and in the host and the device form.  Eigenvalues agree with ek_hip_solve_device's to
 * rounding, not to the bit (QL here, divide & conquer there).
 * An A of any finite magnitude is scaled internally, as in ek_hip_solve_device (by an exact power of two when max|a|
 * lies outside 2^-256 .. 2^256); the d and e left in dA are those of the caller's A.  The scale is taken from A alone:
 * for problem 1, max|a| / lambda_min(B) beyond about 2^500 can still overflow and is reported as 100000 + n + 1.
 * Device form, IN PLACE like ek_hip_solve_device: on return the lower triangle of each A holds what DSYTD2 leaves (d on
 * the diagonal, e below it, the tails of the Householder vectors below that; tau_k = 2 / (1 + |tail_k|^2)), the lower
 * triangle of each B holds L.  The strictly upper triangles of A and B are never read and never written (a NaN there
 * survives bit for bit), nor is anything between the columns (rows n..ld-1) or between the problems.
 * Workspace: batch ints of device memory, kept until ek_hip_finalize. */
#define EK_HIP_BATCH_NMAX 128
int ek_hip_eigenpairs_batched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                     double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                     long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout; A and B are left untouched (the call works on device copies), and so is
 * what lies between the columns and the problems of Z */
int ek_hip_eigenpairs_batched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                              const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                              long long strideZ, int *info, double *seconds);

/* A WINDOW of eigenpairs of every problem of a batch (RANGE 'I' / 'V', as rocSOLVER's syevdx_strided_batched has it): one
 * order 0 <= n <= EK_HIP_BATCH_NMAX and one window for the whole batch, a workgroup per problem from first load to last
 * store.  The reduction is that of ek_hip_eigenpairs_batched*; the implicit QL is replaced by Sturm bisection of the wanted
 * values and inverse iteration (DSTEIN's scheme) for their vectors, and only the window's columns are back-transformed: no
 * full spectrum is computed anywhere.  NOT COLLECTIVE; the call synchronises.  23 arguments:
 *   problem, jobz, dA .. strideB, seconds : exactly as ek_hip_eigenpairs_batched* (a stride of 0 is an argument error; B
 *                   is not looked at for problem 0; lower triangles only)
 *   range         : 0 'I': the indices il .. iu, 1-based, 1 <= il <= iu <= n; vl, vu not referenced
 *                   1 'V': the eigenvalues in the half-open (vl, vu], vl < vu, -Inf / +Inf legal; il, iu not referenced.
 *                   They are counted on the tridiagonal by Sturm counts, the bounds scaled by the exact power of two by
 *                   which the kernel scaled the problem (ek_hip_stebz_range's rule)
 *   m             : out: HOST array of batch ints: the number of pairs problem b returns -- iu - il + 1 for every
 *                   successful problem under 'I', the count under 'V' (it differs from problem to problem; 0 is
 *                   success).  A failed problem gets 0, except under info[b] = -20
 *   dw            : out: batch x n doubles; problem b's m[b] values ascending at dw + b * n, the rest of the row is not
 *                   written
 *   dZ, ldz, zcap, strideZ : out (jobz = 1): problem b's vectors are columns 0 .. m[b] - 1 of the n x zcap array at
 *                   dZ + b * strideZ, ldz >= max(1, n), strideZ >= ldz * max(1, zcap); the columns from m[b] on are
 *                   not written.  Orthonormal, B-orthonormal for problem 1.  'I' needs zcap >= iu - il + 1.  'V' with
 *                   m[b] > zcap: info[b] = -20, m[b] is the count, and nothing of that problem's w or Z is written; the
 *                   other problems are unaffected.  dZ, ldz and strideZ are not referenced when jobz = 0; zcap is
 *                   checked all the same
 *   info          : out: HOST array of batch ints: 0, always with finite w; k > 0 the failing pivot of B and -5 NaN / Inf
 *                   in A's lower triangle, as ek_hip_eigenpairs_batched*; -20 as above; 100000 + n + 1: the reduction
 *                   left a non-finite tridiagonal, or an eigenvalue lies beyond a double; 200000 + k: inverse iteration
 *                   did not converge for the eigenvalue of global index k (5 iterations to meet DSTEIN's growth test,
 *                   then 2 more).  A failed problem writes only its own slots
 * Return value: 0, or -k for argument k of the prototype, decided before any device work without dereferencing a data
 * pointer, the first offending argument deciding: -1 problem, -2 jobz, -3 range, -4 n, -5 batch (n = 0 or batch = 0:
 * success, nothing further looked at); -6 vl NaN, -7 vu NaN or vl >= vu ('V' only); -8 il, -9 iu ('I' only); -10 .. -12 A;
 * -13 .. -15 B (problem 1 only); -16 m; -17 w; -18 Z, -19 ldz and -21 strideZ (jobz = 1 only); -20 zcap < 0 or 'I' with
 * zcap < iu - il + 1; -22 info; <= -1000 HIP runtime error.
 * In place (device form): dA[b] <- DSYTD2's lower layout and dB[b] <- L, bit for bit what
 * ek_hip_eigenpairs_batched_device leaves for the same pair (the stages in front of QL are the same arithmetic); strictly
 * upper triangles, rows n .. ld - 1 and the gaps between the problems are neither read nor written.  The host form leaves
 * A and B untouched, and of w and Z everything the device form does not write.
 * Same bits: the value of index k depends on (n, A, B, k) alone -- not on il / iu, range, jobz, zcap, the batch, the
 * position or the form: every index makes the same bisection passes over one grid that the tridiagonal fixes.  A
 * vector's bits may depend on the window, because its cluster mates inside the window do, and on nothing else.  Values
 * agree with ek_hip_eigenpairs_batched*'s to the bound, not to the bit (bisection here, QL there).
 * A batch runs in chunks of at most K problems, launched one after the other on one stream: K = 1024, or as many slots
 * (below) as fit 256 MiB where that is fewer, in multiples of 256 and at least 512.
 * Workspace (device memory, grown on demand, kept until ek_hip_finalize): 2 batch ints, and for jobz = 1 the LU factors
 * of inverse iteration, min(batch, K) slots of 5 n c doubles, c = iu - il + 1 ('I') or min(zcap, n) ('V'): 655 360 bytes
 * a slot at n = c = 128 (K = 512, 336 MB at most), 81 920 bytes for a window of 16 (K = 1024, 84 MB).  Under 'V' give the
 * zcap that is needed: c follows it.
 * Where it is slow: the vectors of a cluster (gaps <= 1e-3 |T|_1) are formed one after the other, a round each.  A fully
 * clustered problem with all pairs wanted (A = c I at order 128: 128 rounds) costs 16 times the full call of
 * ek_hip_eigenpairs_batched* (two clusters of 64: 5 times), which is then the call to use. */
int ek_hip_eigenpairs_window_batched_device(int problem, int jobz, int range, int n, int batch, double vl, double vu,
                                            int il, int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                            long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                            long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout */
int ek_hip_eigenpairs_window_batched(int problem, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                     int iu, const double *A, int lda, long long strideA, const double *B, int ldb,
                                     long long strideB, int *m, double *w, double *Z, int ldz, int zcap,
                                     long long strideZ, int *info, double *seconds);

/* The window call for orders up to EK_HIP_XBATCH_NMAX.  Argument for argument these are
 * ek_hip_eigenpairs_window_batched_device / ek_hip_eigenpairs_window_batched -- 23 arguments, the same argument-error
 * codes decided before any device work and without dereferencing a data pointer, the first offending argument deciding --
 * with one difference: -4 is for n < 0 or n > EK_HIP_XBATCH_NMAX.
 *   0 <= n <= EK_HIP_BATCH_NMAX : forwarded to the code behind ek_hip_eigenpairs_window_batched*: the same kernel, the
 *                   same bits in m, w, Z, info and the in-place images
 *   EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX : the kernel class of ek_hip_eigenpairs_xbatched* (the n x n image in a
 *                   device workspace) with the same bisection and inverse iteration in place of its QL; the wanted
 *                   vectors are held as rows of the image
 * The whole contract above holds at the new orders: m, info (0 / k > 0 / -5 / -20 / 100000 + n + 1 / 200000 + k), what is
 * written and what is left alone, and the bit contracts -- the value of index k depends on (n, A, B, k) alone; a vector's
 * bits depend on the window only through its cluster mates inside it; after a device call dA and dB are, bit for bit, what
 * ek_hip_eigenpairs_xbatched_device leaves for the same pair; values agree with ek_hip_eigenpairs_xbatched*'s to the bound,
 * not to the bit.
 * Above EK_HIP_BATCH_NMAX a batch runs in chunks of at most K problems on one stream: K = 1024, or as many LU slots as fit
 * 1 GiB where that is fewer, in multiples of 512 (the workgroups the device holds at once, two per compute unit) and at
 * least 512.  Workspace (device memory, grown on demand, kept until ek_hip_finalize): 2 batch ints; min(batch, K) images
 * of 526 336 bytes (shared with ek_hip_eigenpairs_xbatched*: 539 MB at K = 1024); and for jobz = 1 min(batch, K) LU slots
 * of 5 n c doubles, c = iu - il + 1 ('I') or min(zcap, n) ('V'): 2 621 440 bytes at n = c = 256, where K = 512 -- 1.34 GB
 * of LU and 269 MB of images at most; 327 680 bytes for a window of 32 at n = 256 (K = 1024, 336 MB).  Under 'V' give the
 * zcap that is needed: c follows it.
 * Where it is slow: as above, a fully clustered problem with all pairs wanted; ek_hip_eigenpairs_xbatched* is then the
 * call to use. */
int ek_hip_eigenpairs_window_xbatched_device(int problem, int jobz, int range, int n, int batch, double vl, double vu,
                                             int il, int iu, double *dA, int lda, long long strideA, double *dB,
                                             int ldb, long long strideB, int *m, double *dw, double *dZ, int ldz,
                                             int zcap, long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout */
int ek_hip_eigenpairs_window_xbatched(int problem, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                      int iu, const double *A, int lda, long long strideA, const double *B, int ldb,
                                      long long strideB, int *m, double *w, double *Z, int ldz, int zcap,
                                      long long strideZ, int *info, double *seconds);

/* The same call for orders up to EK_HIP_XBATCH_NMAX ("xbatched").  Argument for argument these are
 * ek_hip_eigenpairs_batched_device / ek_hip_eigenpairs_batched -- 16 arguments, the same argument-error codes decided
 * before any device work and without dereferencing a pointer, the first offending argument deciding -- with one
 * difference: -3 is for n < 0 or n > EK_HIP_XBATCH_NMAX.
 *   0 <= n <= EK_HIP_BATCH_NMAX : forwarded to the code behind ek_hip_eigenpairs_batched*: the same kernel, the same bits
 *                   in w, Z, info and the in-place images
 *   EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX : a second kernel class runs the same stages with the same arithmetic
 *                   rules, again one workgroup per problem from first load to last store and no launch between the
 *                   stages, but with the n x n working image in a device workspace instead of LDS
 * The whole contract of ek_hip_eigenpairs_batched* holds at the new orders:
 *   info[b]       : 0 success, always with finite w; k > 0: the 1-based failing pivot of B (a pivot must lie inside
 *                   1e-290 < pivot < 1e290; a NaN in B included); -5: NaN / Inf in the lower triangle of A;
 *                   100000 + k: the QL iteration failed (k = n + 1: the reduction overflowed, or an eigenvalue lies
 *                   beyond the range of a double).  A failed problem writes nothing outside its own slots (whose w and Z
 *                   hold unspecified values); the other problems of the batch are unaffected
 *   scaling       : A is scaled by an exact power of two when max|a| lies outside 2^-256 .. 2^256; the d and e left in
 *                   dA are those of the caller's A
 *   device form   : IN PLACE: the lower triangle of each dA holds DSYTD2's lower layout (d, e, the tails of the
 *                   Householder vectors; tau_k = 2 / (1 + |tail_k|^2)), the lower triangle of each dB holds L.  The
 *                   strictly upper triangles, the rows n..ld-1 and the gaps between the problems are neither read nor
 *                   written.  The host form leaves A and B untouched
 *   same bits     : the same (A, B) gives bit-identical info, w, Z and images alone, at any position of any batch, and
 *                   in the host and the device form
 * A batch of an order above EK_HIP_BATCH_NMAX runs in chunks of at most 1024 problems, launched one after the other on
 * one stream without a host synchronise in between.
 * Workspace: batch ints, and for orders above EK_HIP_BATCH_NMAX min(batch, 1024) images of 256 x 257 doubles (526 336
 * bytes each, 539 MB for 1024 problems or more) of device memory, grown on demand and kept until ek_hip_finalize.
 * The variable-order form at the new orders is ek_hip_eigenpairs_xvbatched* below.  Problem types 2 and 3 at these
 * orders are ek_hip_sygv_xbatched* below.  The acceptance check of these entries is ek_hip_check_xbatched* below. */
#define EK_HIP_XBATCH_NMAX 256
int ek_hip_eigenpairs_xbatched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                      double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                      long long strideZ, int *info, double *seconds);
int ek_hip_eigenpairs_xbatched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                               const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                               long long strideZ, int *info, double *seconds);

/* The same for problems of DIFFERENT orders in one call ("vbatched"): problem b has order n[b], 0 <= n[b] <=
 * EK_HIP_BATCH_NMAX, and its own arrays, named by pointer arrays instead of a base and a stride.
 *   n, lda, ldb, ldz, info and the four pointer arrays dA, dB, dw, dZ are HOST arrays of `batch` entries in both forms;
 *   the pointers IN the pointer arrays are device addresses (device form) or host addresses (host form).
 *   problem, jobz : as above, one value for the whole batch
 *   batch         : >= 0 (0: success, nothing referenced)
 *   n             : n[b] = 0: problem b references nothing (its pointers may be NULL) and gets info[b] = 0
 *   dA, lda       : dA[b]: problem b's column-major n[b] x n[b] A, lda[b] >= max(1, n[b]); lower triangle referenced
 *   dB, ldb       : the same for B; not looked at (may be NULL) when problem = 0
 *   dw            : out: dw[b]: n[b] eigenvalues, ascending
 *   dZ, ldz       : out (jobz = 1): dZ[b]: n[b] x n[b] eigenvectors, ldz[b] >= max(1, n[b]), column k belonging to
 *                   dw[b][k]; not looked at when jobz = 0
 *   info          : out: one int per problem, the codes of ek_hip_eigenpairs_batched* (0; k > 0 failing pivot of B;
 *                   -5 NaN / Inf in A's lower triangle; 100000 + k QL).  A failed problem writes nothing outside its own
 *                   slots; the other problems are unaffected
 *   seconds       : NULL or one double: device time from before the first launch to after the last
 * Return value: 0 when the arguments were legal and the launches ran (whatever info[] says); -k for argument k of this
 * prototype, decided before any device work and without dereferencing any pointer of the pointer arrays, the first
 * offending argument deciding: -4 n NULL or an order outside 0 .. EK_HIP_BATCH_NMAX; -5 / -7 / -9 / -10 array NULL or
 * a NULL entry for a problem of order > 0; -6 / -8 / -11 array NULL or a leading dimension too small; -12 info NULL;
 * <= -1000 HIP runtime error.  The problems must not overlap in memory (not checked).
 * THE SAME BITS AS THE UNIFORM CALL: problem b's w, Z, info and in-place images are bit-identical to what
 * ek_hip_eigenpairs_batched_device returns for the same (n, A, B) alone, wherever the problem sits in the batch and
 * whatever surrounds it.  Every problem runs in the kernel class its own order picks (n <= 32 / 64 / 128); the
 * classes are launched largest first (at most three launches, no host synchronise between them), a class's
 * problems in descending order.
 * NOT COLLECTIVE; the call synchronises.  Device form IN PLACE as above (dA[b] <- DSYTD2's layout, dB[b] <- L; strictly
 * upper triangles and rows n[b] .. ld-1 neither read nor written).  Workspace: batch ints and one 56-byte table entry
 * per problem of device memory, two streams and ten events, kept until ek_hip_finalize. */
int ek_hip_eigenpairs_vbatched_device(int problem, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                      double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                      const int *ldz, int *info, double *seconds);
/* host addresses in A, B, w, Z; A and B are left untouched: the lower triangles travel packed (ld = n[b]) in one copy
 * per matrix kind, and w and Z come back in one copy each.  w[b] and Z[b] of a failed problem are left as they were */
int ek_hip_eigenpairs_vbatched(int problem, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                               const double *const *B, const int *ldb, double *const *w, double *const *Z,
                               const int *ldz, int *info, double *seconds);

/* DSYGV's three problem types for the batched forms -- what itype is to rocSOLVER's / cuSOLVER's sygvd batched calls and
 * what ek_hip_sygvx* is to ek_hip_eigenpairs*:
 *   itype 1: A x = l B x   (C = L^-1 A L^-T, x = L^-T y; X^T B X = I)
 *   itype 2: A B x = l x   (C = L^T A L,     x = L^-T y; X^T B X = I)
 *   itype 3: B A x = l x   (C = L^T A L,     x = L y;    X^T B^-1 X = I)
 * with B = L L^T, one itype for the whole call.  Every other argument is exactly that of ek_hip_eigenpairs_batched* /
 * ek_hip_eigenpairs_vbatched* with problem = 1 (argument k here is argument k there, itype in the place of problem), B is
 * always required, and the same kernel runs: only the reduction to standard form and the recovery depend on the type.
 * Return value: -1 for itype outside 1 .. 3, then the codes of the eigenpairs forms (uniform: -8 / -9 / -10 for B, ldb,
 * strideB; variable: -7 / -8 for dB, ldb), decided before any device work and without dereferencing a data pointer.
 * info[b]: 0; k > 0 the failing pivot of B (the value type 1 reports for that B); -5 NaN / Inf in A's lower triangle;
 * 100000 + k as above; info = 0 always comes with finite w.
 * itype 1 IS ek_hip_eigenpairs_*batched*(problem = 1): the same bits in w, Z, info and the in-place images of dA and dB.
 * Types 2 and 3 return bit-identical w for the same (A, B) and leave the same images: dA[b] <- DSYTD2's layout of
 * C = L^T A L (d and e those of the caller's scaling), dB[b] <- L, the L of type 1.  Their Z are related by Z3 = B Z2 to
 * rounding.  What holds for the eigenpairs forms holds here: the same bits wherever a problem sits and in the host, the
 * device, the uniform and the variable form; strictly upper triangles, rows n .. ld-1 and the gaps between problems are
 * neither read nor written; a failed problem touches its own slots only.
 * A of any finite magnitude is scaled as above, from A alone.  For types 2 and 3 the reduction amplifies by lambda_max(B)
 * where type 1's amplifies by 1 / lambda_min(B): max|a| lambda_max(B) beyond about 2^500 can overflow and is reported as
 * 100000 + n + 1, never as info = 0.
 * ek_hip_check_batched* / ek_hip_check_vbatched* below remain checks of type 1 (and of the standard problem), with the
 * reference verifier's normalisations; ek_hip_check_sygv_batched* / ek_hip_check_sygv_vbatched* behind them carry those
 * normalisations over to types 2 and 3, and ek_hip_check_sygvx* does the same for one problem of any order. */
int ek_hip_sygv_batched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                               double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                               long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout; A and B are left untouched (the call works on device copies) */
int ek_hip_sygv_batched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                        const double *B, int ldb, long long strideB, double *w, double *Z, int ldz, long long strideZ,
                        int *info, double *seconds);
int ek_hip_sygv_vbatched_device(int itype, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                const int *ldz, int *info, double *seconds);
/* host addresses in A, B, w, Z; A and B are left untouched; w[b] and Z[b] of a failed problem are left as they were */
int ek_hip_sygv_vbatched(int itype, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                         const double *const *B, const int *ldb, double *const *w, double *const *Z, const int *ldz,
                         int *info, double *seconds);

/* Problems of DIFFERENT orders up to EK_HIP_XBATCH_NMAX in one call ("xvbatched"): what ek_hip_eigenpairs_xbatched* are
 * to ek_hip_eigenpairs_batched*, for ek_hip_eigenpairs_vbatched* and ek_hip_sygv_vbatched*.  The same 13 arguments, host
 * and device conventions, argument-error codes (decided before any device work and without dereferencing a pointer of
 * the pointer arrays, the first offending argument deciding) and contract as the entries they extend, with one
 * difference: -4 is for n NULL or an order outside 0 .. EK_HIP_XBATCH_NMAX.  ek_hip_eigenpairs_vbatched* and
 * ek_hip_sygv_vbatched* keep answering -4 above EK_HIP_BATCH_NMAX.  For the sygv forms -1 is for itype outside 1 .. 3 and B
 * is always required (-7 / -8).
 * Problem b runs in the kernel its own order picks: n[b] <= 32 / 64 / 128 the classes of ek_hip_*_vbatched*,
 * EK_HIP_BATCH_NMAX < n[b] <= EK_HIP_XBATCH_NMAX the kernel of ek_hip_*_xbatched* (image in device memory).
 * THE SAME BITS AS THE UNIFORM CALL: problem b's w, Z, info and in-place images of dA and dB are bit-identical to what
 * ek_hip_eigenpairs_xbatched_device (ek_hip_sygv_xbatched_device) returns for the same (n, A, B) alone, wherever the
 * problem sits, whatever surrounds it, in whichever chunk, and in the host and the device form.  So a batch with no order
 * above EK_HIP_BATCH_NMAX returns the bits of ek_hip_*_vbatched*, and ek_hip_sygv_xvbatched*(itype = 1) those of
 * ek_hip_eigenpairs_xvbatched*(problem = 1).
 * Everything else carries over: info[b] is 0 (always with finite w), the failing pivot of B, -5 or 100000 + k; a failed
 * problem touches only its own slots; strictly upper triangles, rows n[b] .. ld-1 and whatever lies between problems are
 * neither read nor written; A is scaled from A alone; types 2 and 3 give equal w and equal dA bits for the same (A, B);
 * the problems must not overlap in memory (not checked); NOT COLLECTIVE; the call synchronises.
 * The classes are launched largest first, a class's problems in descending order; the class above EK_HIP_BATCH_NMAX runs
 * on the context's stream in chunks of at most 1024 problems, one after the other, the other classes beside it on
 * streams of their own.  Workspace: that of ek_hip_*_vbatched* (three streams and thirteen events), and, only when an
 * order above EK_HIP_BATCH_NMAX is present, min(problems above EK_HIP_BATCH_NMAX, 1024) images as for
 * ek_hip_eigenpairs_xbatched*; kept until ek_hip_finalize.
 * The acceptance checks of these entries' results, in the form they come in, are ek_hip_check_xvbatched* and
 * ek_hip_check_sygv_xvbatched* below (ek_hip_check_*vbatched* stop at EK_HIP_BATCH_NMAX). */
int ek_hip_eigenpairs_xvbatched_device(int problem, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                       double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                       const int *ldz, int *info, double *seconds);
/* host addresses in A, B, w, Z, as ek_hip_eigenpairs_vbatched: A and B are left untouched, the lower triangles travel
 * packed (ld = n[b]) in one copy per matrix kind, w and Z come back in one copy each; w[b] and Z[b] of a failed problem
 * are left as they were */
int ek_hip_eigenpairs_xvbatched(int problem, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                                const double *const *B, const int *ldb, double *const *w, double *const *Z,
                                const int *ldz, int *info, double *seconds);
int ek_hip_sygv_xvbatched_device(int itype, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                 double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                 const int *ldz, int *info, double *seconds);
int ek_hip_sygv_xvbatched(int itype, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                          const double *const *B, const int *ldb, double *const *w, double *const *Z, const int *ldz,
                          int *info, double *seconds);

/* DSYGV's three problem types for orders up to EK_HIP_XBATCH_NMAX: what ek_hip_eigenpairs_xbatched* are to
 * ek_hip_eigenpairs_batched*, for ek_hip_sygv_batched*.  The same 16 arguments and argument-error codes as
 * ek_hip_sygv_batched*, decided before any device work and without dereferencing a data pointer, the first offending
 * argument deciding: -1 for itype outside 1 .. 3 (B always required: -8 / -9 / -10), -3 for n < 0 or n > EK_HIP_XBATCH_NMAX.
 *   0 <= n <= EK_HIP_BATCH_NMAX : forwarded to the code behind ek_hip_sygv_batched*: the same bits in w, Z, info, dA and dB
 *   EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX, itype 1 : ek_hip_eigenpairs_xbatched*(problem = 1) to the bit (the same
 *                   kernel)
 *   EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX, itype 2, 3 : a second instantiation of that kernel with the reduction
 *                   C = L^T A L and, for type 3, the recovery x = L y; every other stage is the same code
 * The contract of ek_hip_sygv_batched* and of ek_hip_eigenpairs_xbatched* holds for types 2 and 3 at the new orders:
 * info[b] is 0 (always with finite w), the failing pivot k of B (the value type 1 reports), -5 or 100000 + k; A is scaled
 * from A alone; the device form works IN PLACE, dA[b] <- DSYTD2's lower layout of C = L^T A L (d and e those of the
 * caller's scaling), dB[b] <- L, type 1's L bit for bit; types 2 and 3 return the same w and the same dA image bit for
 * bit and Z3 = B Z2 to rounding; jobz = 0 returns the bits of jobz = 1 in w and dA; the same bits alone, at any position of
 * any batch, in any chunk and in the host and the device form; strictly upper triangles, rows n .. ld-1 and the gaps
 * between problems are neither read nor written; a failed problem touches its own slots only.  Chunks and workspace are
 * those of ek_hip_eigenpairs_xbatched*.  ek_hip_sygv_batched* keep answering -3 above EK_HIP_BATCH_NMAX.
 * The variable-order form above EK_HIP_BATCH_NMAX is ek_hip_sygv_xvbatched* below.  ek_hip_check_xbatched* stays a check of type 1; the
 * acceptance check of these entries, all three types, is ek_hip_check_sygv_xbatched* below. */
int ek_hip_sygv_xbatched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout; A and B are left untouched (the call works on device copies) */
int ek_hip_sygv_xbatched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                         const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                         long long strideZ, int *info, double *seconds);

/* The same calls for orders up to EK_HIP_YBATCH_NMAX ("ybatched").  Argument for argument these are
 * ek_hip_eigenpairs_xbatched* and ek_hip_sygv_xbatched* -- 16 arguments, the same argument-error codes decided before any
 * device work and without dereferencing a data pointer, the first offending argument deciding (-1 for an itype outside
 * 1 .. 3 before everything else, B always required in the sygv form) -- with one difference: -3 is for n < 0 or
 * n > EK_HIP_YBATCH_NMAX.
 *   0 <= n <= EK_HIP_XBATCH_NMAX : forwarded to the code behind the xbatched entries: the same bits in info, w, Z, dA, dB
 *   EK_HIP_XBATCH_NMAX < n <= EK_HIP_YBATCH_NMAX : a second class of the xbatched kernel (512 rows, 1024 threads, two
 *                   threads per row, the image with leading dimension 513 in the device workspace) runs the same stages
 *                   with the same arithmetic rules and ownership maps; ek_hip_sygv_ybatched*(itype = 1) is
 *                   ek_hip_eigenpairs_ybatched*(problem = 1) to the bit, types 2 and 3 run the instantiation with the
 *                   reduction C = L^T A L
 * The whole contract of ek_hip_eigenpairs_xbatched* and ek_hip_sygv_xbatched* holds at the new orders: the info codes;
 * scaling taken from A alone; the device form IN PLACE (DSYTD2's lower layout in dA, L in dB); strictly upper triangles,
 * rows n .. ld-1 and gaps never read or written; a failed problem touches only its own slots; the same bits alone, at any
 * position of any batch, in any chunk, in the host and the device form; types 2 and 3 share w and dA bit for bit and
 * Z3 = B Z2 to rounding; jobz = 0 returns the bits of jobz = 1 in w and dA.
 * A batch of an order above EK_HIP_XBATCH_NMAX runs in chunks of at most 256 problems (one workgroup of 1024 threads per
 * compute unit; ek_hip_debug_ybatched_chunk), launched one after the other on one stream without a host synchronise.
 * Workspace: batch ints, and for orders above EK_HIP_XBATCH_NMAX min(batch, 256) images of 512 x 513 doubles (2 101 248
 * bytes each, 538 MB for 256 problems or more) of device memory.  It is the allocation of ek_hip_eigenpairs_xbatched*,
 * sized in bytes for whichever class asked for more: grown on demand, kept until ek_hip_finalize.
 * The xbatched and batched entries keep answering -3 where they did.  Not at these orders: the variable-order form, the
 * windows and the batched checks (ek_hip_check*, ek_hip_check_sygvx_device take any order, one problem a call). */
#define EK_HIP_YBATCH_NMAX 512
int ek_hip_eigenpairs_ybatched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                      double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                      long long strideZ, int *info, double *seconds);
int ek_hip_eigenpairs_ybatched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                               const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                               long long strideZ, int *info, double *seconds);
int ek_hip_sygv_ybatched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                long long strideZ, int *info, double *seconds);
int ek_hip_sygv_ybatched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                         const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                         long long strideZ, int *info, double *seconds);

/* A WINDOW of eigenpairs of DSYGV's three problem types, per problem of a batch -- what itype is to rocSOLVER's
 * sygvdx_strided_batched, and what ek_hip_sygv_batched* are to ek_hip_eigenpairs_batched*, for
 * ek_hip_eigenpairs_window_batched* / ek_hip_eigenpairs_window_xbatched*.  The 23 arguments of those entries with problem
 * = 1 (argument k here is argument k there, itype in the place of problem); B is always required.
 * Return value: -1 for itype outside 1 .. 3 first, then the window entries' codes -2 .. -22 (B: -13 / -14 / -15 for every
 * type), decided before any device work and without dereferencing a data pointer; n = 0 or batch = 0: 0, nothing touched.
 * -4 is for n > EK_HIP_BATCH_NMAX (the batched pair) or n > EK_HIP_XBATCH_NMAX (the xbatched pair, which forwards
 * n <= EK_HIP_BATCH_NMAX to the code behind the batched pair: the same bits).
 * itype 1 IS ek_hip_eigenpairs_window_batched* / ek_hip_eigenpairs_window_xbatched* with problem = 1: the same bits in m,
 * info, w, Z, dA and dB.
 * Types 2 and 3 run an instantiation of the window kernels with the reduction C = L^T A L in place of type 1's (stages 0
 * to 3 are those of ek_hip_sygv_batched* / ek_hip_sygv_xbatched*, stage 4W is the window entries'), and recover
 * x = L^-T y (type 2) or x = L y (type 3) on the window's columns alone:
 *   values        : the eigenvalue of index k is the same bits in both types and m[b] under 'V' is the same; it depends on
 *                   (n, A, B, k) alone -- not on the window, range, jobz, zcap, the batch, the position, the chunk or the
 *                   form.  'V' counts the eigenvalues of C = L^T A L, the bounds scaled by the exact power of two of the
 *                   kernel's scaling as in the window entries
 *   images        : after a device call dA and dB are, bit for bit, what ek_hip_sygv_batched_device /
 *                   ek_hip_sygv_xbatched_device leave for the same pair and type; dB is type 1's L
 *   vectors       : type 2's are B-orthonormal, type 3's B^-1-orthonormal, and Z3 = B Z2 to rounding, column by column
 * m, info (0, the failing pivot k, -5, -20, 100000 + n + 1, 200000 + k), the isolation of a failed problem, what is written
 * (m[b] values of a row of w, m[b] columns of Z; nothing of w or Z under -20) and what is neither read nor written (upper
 * triangles, rows n .. ld - 1, gaps; A and B in the host forms) are the window entries'.  So are the chunk rule and the
 * workspace: see ek_hip_eigenpairs_window_batched* and, above EK_HIP_BATCH_NMAX, ek_hip_eigenpairs_window_xbatched*.
 * ek_hip_eigenpairs_window_*batched* themselves stay type 1 only (problem = 2 is -1 there). */
int ek_hip_sygv_window_batched_device(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                      int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                      long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                      long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout */
int ek_hip_sygv_window_batched(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il, int iu,
                               const double *A, int lda, long long strideA, const double *B, int ldb, long long strideB,
                               int *m, double *w, double *Z, int ldz, int zcap, long long strideZ, int *info,
                               double *seconds);
int ek_hip_sygv_window_xbatched_device(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                       int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                       long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                       long long strideZ, int *info, double *seconds);
/* host arrays A, B, w, Z with the same layout */
int ek_hip_sygv_window_xbatched(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il, int iu,
                                const double *A, int lda, long long strideA, const double *B, int ldb,
                                long long strideB, int *m, double *w, double *Z, int ldz, int zcap, long long strideZ,
                                int *info, double *seconds);

/* A WINDOW of eigenpairs PER PROBLEM for problems of DIFFERENT orders up to EK_HIP_XBATCH_NMAX in one call -- what
 * ek_hip_*_xvbatched* are to ek_hip_*_xbatched*, for ek_hip_eigenpairs_window_xbatched* and ek_hip_sygv_window_xbatched*.
 * Twenty arguments.  problem (itype), jobz (0 / 1) and range (0 = 'I', 1 = 'V') are one value for the call; everything else
 * is per problem.  n, vl, vu, il, iu, lda, ldb, m, ldz, zcap, info and the four pointer arrays are HOST arrays of `batch`
 * entries in both forms; the pointers inside dA, dB, dw, dZ are device addresses in the device form and host addresses in
 * the host form.  Problem b: order n[b], the window il[b] .. iu[b] ('I'; vl, vu not looked at, may be NULL) or
 * (vl[b], vu[b]] ('V'; il, iu not looked at, may be NULL), dw[b] with room for n[b] doubles of which m[b] are written,
 * dZ[b] n[b] x zcap[b] with ldz[b] >= max(1, n[b]) of which the columns 0 .. m[b]-1 are written.
 * Return value: 0, or -k for argument k, decided before any device work and without dereferencing a pointer of the pointer
 * arrays, the first offending argument deciding; per-problem conditions hold for the problems of order > 0:
 *   -1 problem (itype outside 1 .. 3, first)   -2 jobz   -3 range   -4 batch < 0 (batch = 0: 0, nothing looked at)
 *   -5 n NULL or an order outside 0 .. EK_HIP_XBATCH_NMAX
 *   -6 vl NULL or a NaN, -7 vu NULL, a NaN or vl[b] >= vu[b] ('V' only)
 *   -8 il NULL or il[b] outside 1 .. n[b], -9 iu NULL or iu[b] outside il[b] .. n[b] ('I' only)
 *   -10 / -11 A / lda   -12 / -13 B / ldb (problem 1; always for the sygv forms)   -14 m   -15 dw
 *   -16 / -17 Z / ldz (jobz = 1 only; dZ[b] may be NULL where zcap[b] = 0)
 *   -18 zcap NULL, zcap[b] < 0, or 'I' with zcap[b] < iu[b] - il[b] + 1 (with and without vectors)   -19 info
 *   <= -1000 a HIP runtime error
 * n[b] = 0 references nothing and gets info[b] = 0, m[b] = 0; a batch of nothing but empty problems is filled on the host.
 * THE SAME BITS AS THE UNIFORM CALL: problem b's m, info, w[0 .. m), Z[:, 0 .. m) and the in-place images of dA[b] and dB[b]
 * are bit for bit what ek_hip_eigenpairs_window_xbatched_device (ek_hip_sygv_window_xbatched_device) returns for
 * (n[b], A, B, window b, zcap[b]) alone -- wherever the problem sits, whatever surrounds it, in whichever launch, under
 * either setting of ek_hip_debug_vbatched_streams, in the host and the device form.  So the value of index k depends on
 * (n, A, B, k) alone, itype = 1 is the eigenpairs entry with problem = 1, and types 2 and 3 share w and m.
 * info[b] and m[b] are the uniform window call's: 0 (always with finite w), the failing pivot of B, -5, -20 ('V' with
 * m[b] > zcap[b] under jobz = 1: m[b] is the count, nothing of that problem's w or Z is written), 100000 + n[b] + 1,
 * 200000 + k.  A failed problem touches only its own slots.  Strictly upper triangles, rows n[b] .. ld-1, the rest of w[b],
 * the columns of Z[b] from m[b] on and whatever lies between problems are neither read nor written.  The problems must not
 * overlap in memory (not checked); NOT COLLECTIVE; the call synchronises; *seconds (may be NULL) is the device time from
 * before the first launch to after the last.
 * Problem b runs in the class its order picks (256 / 128 / 64 / 32), the classes largest first beside each other on streams
 * of their own, a class's problems in descending order.  A class runs in launches of consecutive problems: a launch ends at
 * 1024 problems (ek_hip_debug_window_batched_chunk, ek_hip_debug_window_xbatched_chunk) or where the LU slots of inverse
 * iteration (5 n[b] wcols[b] doubles, wcols[b] = iu[b]-il[b]+1 or min(zcap[b], n[b]); jobz = 1) would pass the class's
 * budget: 1 GiB above EK_HIP_BATCH_NMAX, 256 MiB shared in equal parts by the classes present below it.  Workspace: the
 * widest launch of every class in LU slots, an image per problem of the widest launch above EK_HIP_BATCH_NMAX, two tables
 * and two words per problem; kept until ek_hip_finalize. */
int ek_hip_eigenpairs_window_xvbatched_device(int problem, int jobz, int range, int batch, const int *n, const double *vl,
                                              const double *vu, const int *il, const int *iu, double *const *dA,
                                              const int *lda, double *const *dB, const int *ldb, int *m,
                                              double *const *dw, double *const *dZ, const int *ldz, const int *zcap,
                                              int *info, double *seconds);
/* host addresses in A, B, w, Z: A and B are left untouched, their lower triangles travel packed (ld = n[b]) in one copy per
 * matrix kind, and only what the kernel wrote comes back: m[b] values of w[b], m[b] columns of Z[b], of the problems with
 * info[b] = 0 */
int ek_hip_eigenpairs_window_xvbatched(int problem, int jobz, int range, int batch, const int *n, const double *vl,
                                       const double *vu, const int *il, const int *iu, const double *const *A,
                                       const int *lda, const double *const *B, const int *ldb, int *m, double *const *w,
                                       double *const *Z, const int *ldz, const int *zcap, int *info, double *seconds);
int ek_hip_sygv_window_xvbatched_device(int itype, int jobz, int range, int batch, const int *n, const double *vl,
                                        const double *vu, const int *il, const int *iu, double *const *dA,
                                        const int *lda, double *const *dB, const int *ldb, int *m, double *const *dw,
                                        double *const *dZ, const int *ldz, const int *zcap, int *info, double *seconds);
int ek_hip_sygv_window_xvbatched(int itype, int jobz, int range, int batch, const int *n, const double *vl,
                                 const double *vu, const int *il, const int *iu, const double *const *A, const int *lda,
                                 const double *const *B, const int *ldb, int *m, double *const *w, double *const *Z,
                                 const int *ldz, const int *zcap, int *info, double *seconds);

/* The acceptance checks and the inverse participation ratios of EVERY problem of a batch -- what ek_hip_residual_device,
 * ek_hip_orthogonality_device and ek_hip_ipratios_device are to one problem, with the same normalisations (the
 * reference's: verifier.f90:75-204, :233-330, distribute_matrix.f90:18-78), for the eigenpairs that
 * ek_hip_eigenpairs_batched* / ek_hip_eigenpairs_vbatched* return.  One kernel launch per call (uniform form), at most
 * three (variable form: one per kernel class present, largest class first, descending order inside a class); a
 * workgroup owns a problem from its first load to its last store.  NOT COLLECTIVE; the calls synchronise.
 * Per problem, all n columns checked, A and B symmetric by their lower triangles (as PDSYMM('L','L')):
 *   out[4 b + 0]  a_norm         ||A||_F
 *   out[4 b + 1]  res_ave        sum_j ||r_j||_2 / a_norm / n,  r_j = A z_j - w_j B z_j  (B = I for problem 0)
 *   out[4 b + 2]  res_max        max_j ||r_j||_2 / a_norm
 *   out[4 b + 3]  orthogonality  || D^-1/2 G D^-1/2 with zero diagonal ||_F, G = Z^T B Z, D = diag(G): scaled by the
 *                                computed G_jj, the reference's quirk
 *   ipr           ipr_j = sum_i z_ij^4 / G_jj^2
 * Arguments: problem, n, batch, lda / ldb / ldz, strideA / strideB / strideZ and the layouts are those of
 * ek_hip_eigenpairs_batched* (0 <= n <= EK_HIP_BATCH_NMAX; a stride of 0 is an argument error; dB, ldb, strideB not
 * looked at for problem 0; n = 0 or batch = 0: success, nothing referenced and nothing written, `out` included).
 *   dA, dB        : in: the ORIGINAL matrices.  ek_hip_eigenpairs_batched_device overwrites its dA and dB, so a caller of
 *                   the device forms keeps copies for this call.  Only the lower triangles are referenced; strictly
 *                   upper triangles and the rows n..ld-1 of a column are never read (a NaN there shows nowhere)
 *   dw, dZ        : in: the eigenvalues (batch x n, problem b at dw + b * n) and eigenvectors of the solver entries
 *   info          : HOST array of batch ints or NULL.  NULL: every problem is checked.  Otherwise a problem with
 *                   info[b] != 0 is skipped: its four out slots receive NaN, its ipr slots are left as they were, its w
 *                   and Z are not read by the kernel
 *   out           : HOST array, batch * EK_HIP_CHECK_NOUT doubles
 *   ipr           : HOST array of batch x n doubles (problem b at ipr + b * n), or NULL
 *   seconds       : NULL or one double: device time from before the first launch to after the last
 * Divisions are plain IEEE, as in the one-problem entries: a zero A gives NaN or Inf in the residual slots, a zero
 * column of Z NaN in orthogonality and in its own ipr slot, NaN or Inf in a problem's w or Z shows in that problem's
 * outputs only; none of it changes the return value.
 * Return value: 0 when the arguments were legal and the launches ran; -k for argument k of the prototype, the first
 * offending argument deciding, decided before any device work and without dereferencing any data pointer (info = NULL
 * and ipr = NULL are legal, out = NULL is -15); <= -1000 HIP runtime error.
 * THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on (n, A, B, w, Z) alone -- alone, at any position
 * of any batch, in the uniform and the variable form, in the host and the device form.  The call writes only out and
 * ipr: A, B, w and Z are const and come back bit for bit.
 * Workspace (device memory, kept until ek_hip_finalize): n^2 doubles per checked problem of a generalized batch (S = B Z;
 * none for problem 0), 4 + n doubles per problem for the outputs, 4 bytes (uniform form with skipped problems) or one
 * 72-byte table entry (variable form) per checked problem, two events. */
#define EK_HIP_CHECK_NOUT 4   /* out + 4*b: a_norm, res_ave, res_max, orthogonality of problem b */
int ek_hip_check_batched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                double *seconds);
/* host arrays A, B, w, Z with the same layout (the call works on device copies; the caller's arrays are untouched) */
int ek_hip_check_batched(int problem, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                         int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                         const int *info, double *out, double *ipr, double *seconds);
/* The same checks for orders up to EK_HIP_XBATCH_NMAX, behind ek_hip_eigenpairs_xbatched*.  Argument for argument these are
 * ek_hip_check_batched_device / ek_hip_check_batched -- 17 arguments, the same argument-error codes decided before any device
 * work and without dereferencing a data pointer, the first offending argument deciding -- with one difference: -2 is for
 * n < 0 or n > EK_HIP_XBATCH_NMAX.
 *   0 <= n <= EK_HIP_BATCH_NMAX : forwarded to the code behind ek_hip_check_batched*: the same kernel, the same bits in out
 *                   and ipr
 *   EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX : a kernel class of its own, again one workgroup per problem from first load
 *                   to last store: A Z, S = B Z and G = Z^T S on the fp64 matrix cores over LDS-staged tiles, Z and S in
 *                   device memory instead of LDS
 * The whole contract above holds at the new orders: the same quantities in the same slots, A and B symmetric by their
 * lower triangles (strictly upper triangles, rows n..ld-1 and the gaps between problems are never read), info = NULL checks
 * every problem and a problem with info[b] != 0 gets NaN in its four slots, keeps its ipr slots and has its w and Z left
 * unread, ipr = NULL is legal, out = NULL is -15, n = 0 or batch = 0 returns 0 with nothing referenced or written, plain
 * IEEE divisions, a maximum that keeps a NaN.  THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on
 * (n, A, B, w, Z) alone -- alone, at any position of any batch, in any chunk, in the host and the device form.  A, B, w and
 * Z are const and come back bit for bit.  NOT COLLECTIVE; the calls synchronise.
 * A batch of an order above EK_HIP_BATCH_NMAX runs in chunks of at most 1024 checked problems, launched one after the other
 * on one stream without a host synchronise in between.
 * Workspace above EK_HIP_BATCH_NMAX (device memory, grown on demand, kept until ek_hip_finalize): n^2 doubles for each of the
 * min(checked problems, 1024) problems of a chunk of a generalized batch (S = B Z; at most 512 MiB; none for problem 0),
 * 4 + n doubles per problem for the outputs, 4 bytes per checked problem when some are skipped, two events.
 * The variable-order form at these orders is ek_hip_check_xvbatched* below (the results of ek_hip_eigenpairs_xvbatched* in
 * one call).  The checks of types 2 and 3 at these orders are ek_hip_check_sygv_xbatched* below. */
int ek_hip_check_xbatched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                 const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                 int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                 double *seconds);
/* host arrays A, B, w, Z with the same layout (the call works on device copies; the caller's arrays are untouched) */
int ek_hip_check_xbatched(int problem, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                          int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                          const int *info, double *out, double *ipr, double *seconds);
/* The same checks for a WINDOW of eigenpairs per problem, behind ek_hip_eigenpairs_window_xbatched* (RANGE 'I' / 'V'), every
 * order 0 .. EK_HIP_XBATCH_NMAX: problem b holds c = m[b] pairs, and the c columns are what is checked.  Nineteen arguments;
 * the layouts are exactly what ek_hip_eigenpairs_window_xbatched* returns, so that its m, dw, dZ and info can be handed over
 * unchanged:
 *   m, info       : HOST arrays of batch ints (info may be NULL: no problem is skipped)
 *   dw            : problem b's values are dw[b * n .. b * n + m[b])
 *   dZ            : problem b's vectors are the columns 0 .. m[b]-1 of the n x zcap array at dZ + b * strideZ
 *   dA, dB        : the ORIGINAL matrices, lower triangles only; dB, ldb, strideB are not looked at for problem 0
 *   out           : HOST, batch * EK_HIP_CHECK_NOUT doubles
 *   ipr           : HOST or NULL, batch x n with problem b at ipr + b * n: m[b] entries are written, the rest of the row is
 *                   left as it was
 * Per checked problem, with c = m[b], the quantities of ek_hip_check_sygvx_device(1, n, n_cols = c) and of the reference's
 * verifier with n_check = c:
 *   out[4 b + 0]  ||A||_F
 *   out[4 b + 1]  sum_{j < c} ||r_j||_2 / a_norm / c,  r_j = A z_j - w_j B z_j  (B = I for problem 0)
 *   out[4 b + 2]  max_{j < c} ||r_j||_2 / a_norm; the maximum keeps a NaN
 *   out[4 b + 3]  || D^-1/2 G D^-1/2 with zero diagonal ||_F, G = Z^T B Z of order c, scaled by the computed G_jj
 *   ipr_j         sum_i z_ij^4 / G_jj^2 for j < c
 * Divisions are plain IEEE, as in the entries above.
 * SKIPPED PROBLEMS: with info != NULL and info[b] != 0 the four slots get NaN, the ipr row is left alone, and nothing of the
 * problem's m, w, Z is looked at -- -20 included, where m[b] is a count larger than zcap.  EMPTY WINDOWS: m[b] == 0 (an empty
 * 'V' window) is handled the same way: four NaN, the ipr row left alone, nothing read.  A batch in which every problem is
 * skipped or empty is filled on the host without touching the device.
 * NEVER READ: w from m[b] on, the columns of Z from m[b] on, strictly upper triangles, rows n .. ld-1 and the gaps between
 * problems of the device form (a NaN there shows nowhere).  NEVER WRITTEN: A, B, w, Z are const and come back bit for bit.
 * Return value: 0, or -k for argument k of the prototype, the first offender deciding, before any device work and without
 * dereferencing a data pointer (m and info are host arrays and are read):
 *   -1 problem   -2 n outside 0 .. EK_HIP_XBATCH_NMAX   -3 batch < 0 (n = 0 or batch = 0: 0, nothing referenced or written)
 *   -4 / -5 / -6 A NULL, lda < n, strideA < lda n   -7 / -8 / -9 the same for B (problem 1 only)
 *   -10 m NULL, or m[b] outside 0 .. n for a problem that info does not skip   -11 w NULL   -12 Z NULL   -13 ldz < n
 *   -14 zcap < 0, or zcap < m[b] of a problem that info does not skip   -15 strideZ < ldz max(1, zcap)   -17 out NULL
 *   info, ipr, seconds may be NULL;   <= -1000 a HIP runtime error
 * THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on (problem, n, A, B, m[b], w[0 .. m), Z[:, 0 .. m))
 * alone -- not on zcap, ldz, the strides, the other problems' m, the batch, the position, the chunk or the form: loop
 * bounds from (n, m[b]), fixed summation orders, no atomics.  With m[b] = n the outputs agree with ek_hip_check_xbatched* to
 * rounding, not to the bit (at orders up to EK_HIP_BATCH_NMAX that entry sums in another order).
 * One kernel class serves every order: a workgroup of 512 threads per problem from first load to last store, A Z, S = B Z
 * (over the c columns) and G = Z^T S (c x c) on the fp64 matrix cores over LDS-staged tiles.  The problems run by descending
 * m[b], in chunks of at most 1024 checked problems (ek_hip_debug_check_xbatched_chunk governs it) launched one after the
 * other on one stream.  NOT COLLECTIVE; the call synchronises; *seconds is the device time from before the first launch to
 * after the last.
 * Workspace (device memory of the pool of all ek_hip_check_*batched* entries, kept until ek_hip_finalize): n x max m[b]
 * doubles for each of the min(checked problems, 1024) problems of a chunk of a generalized batch (S = B Z), 4 + n doubles
 * per problem for the outputs, 8 bytes per checked problem, two events.
 * The variable-order form behind ek_hip_*_window_xvbatched* is ek_hip_check_window_xvbatched* below.  DSYGV's types 2 and 3
 * are ek_hip_check_sygv_window_xbatched* below. */
int ek_hip_check_window_xbatched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                        const double *dB, int ldb, long long strideB, const int *m, const double *dw,
                                        const double *dZ, int ldz, int zcap, long long strideZ, const int *info,
                                        double *out, double *ipr, double *seconds);
/* host arrays A, B, w, Z with the same layout (the call works on device copies; the caller's arrays are untouched) */
int ek_hip_check_window_xbatched(int problem, int n, int batch, const double *A, int lda, long long strideA,
                                 const double *B, int ldb, long long strideB, const int *m, const double *w,
                                 const double *Z, int ldz, int zcap, long long strideZ, const int *info, double *out,
                                 double *ipr, double *seconds);
/* The window check for DSYGV's three types, behind ek_hip_sygv_window_xbatched* and ek_hip_sygv_window_batched*, every order
 * 0 .. EK_HIP_XBATCH_NMAX: the nineteen arguments of ek_hip_check_window_xbatched* with itype (1: A x = l B x, 2: A B x = l x,
 * 3: B A x = l x) in the place of problem, the same layouts, so that the solvers' m, dw, dZ and info are handed over
 * unchanged.  dA and dB are the ORIGINAL matrices, lower triangles only (the solvers overwrite theirs: keep copies); dB is
 * required for every type.
 * itype = 1 IS ek_hip_check_window_xbatched*(problem = 1): the same kernel, the same bits.  For types 2 and 3, per checked
 * problem with c = m[b] and B = L L^T, the quantities of ek_hip_check_sygv_xbatched* on c columns:
 *   out[4 b + 0]  ||A||_F ||B||_F
 *   out[4 b + 1]  sum_{j < c} rho_j / c,  rho_j = ||r_j||_2 / (||A||_F ||B||_F ||z_j||_2),
 *                 r_j = A (B z_j) - w_j z_j (type 2), B (A z_j) - w_j z_j (type 3)
 *   out[4 b + 2]  max_{j < c} rho_j; the maximum keeps a NaN
 *   out[4 b + 3]  || D^-1/2 G D^-1/2 with zero diagonal ||_F, G of order c, scaled by the computed G_jj:
 *                 G = Z^T B Z (type 2), (L^-1 Z)^T (L^-1 Z) (type 3)
 *   ipr_j         sum_i z_ij^4 / G_jj^2 for j < c; the rest of the row is left as it was
 * Divisions are plain IEEE.
 * TYPE 3'S FACTOR: the kernel factors the caller's original B itself.  A pivot that is not positive and finite gives NaN in
 * slot 3 and in the m[b] IPR slots of that problem; its residual slots stay valid and the return value stays 0.
 * SKIPPED PROBLEMS (info[b] != 0, -20 with m[b] > zcap included) and EMPTY WINDOWS (m[b] == 0): four NaN, the ipr row left
 * alone, nothing of the problem read; a batch of nothing else is filled on the host without touching the device.
 * NEVER READ: w and the columns of Z from m[b] on, strictly upper triangles, rows n .. ld-1, the gaps between problems.
 * NEVER WRITTEN: A, B, w, Z.
 * Return value: -1 itype outside 1 .. 3 (before everything else); then the codes of ek_hip_check_window_xbatched* with
 * problem = 1: -2 n, -3 batch (n = 0 or batch = 0: 0, nothing referenced or written), -4 / -5 / -6 A, -7 / -8 / -9 B (every
 * type), -10 m, -11 w, -12 Z, -13 ldz, -14 zcap, -15 strideZ, -17 out; the first offender decides, before any device work
 * and without dereferencing a data pointer (m and info are host arrays and are read); <= -1000 a HIP runtime error.
 * THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on (itype, n, A, B, m[b], w[0 .. m), Z[:, 0 .. m)) alone,
 * not on zcap, ldz, the strides, the other problems, the batch, the position, the chunk or the form.  For the same
 * (B, Z, m[b]) slot 3 and the IPRs of type 2 are the bits of the type-1 call.  With m[b] = n the outputs agree with
 * ek_hip_check_sygv_xbatched* to rounding, not to the bit.
 * One kernel class per type serves every order: a workgroup of 512 threads per problem, the products (n^2 c each) on the
 * fp64 matrix cores over LDS-staged tiles; type 3's factor costs n^3 / 3 whatever c is, its forward solve runs over the c
 * columns with 512 / (the power of two >= max(c, 16)) threads per column.  Chunks and *seconds as above.
 * Workspace (the same pool): per problem of a chunk n x max m[b] doubles (type 2), n^2 + n x max m[b] (type 3).
 * Not offered: a variable-order form of this strided prototype.  Problems of different orders (what
 * ek_hip_sygv_window_xvbatched* returns) are checked in one call by ek_hip_check_sygv_window_xvbatched* below. */
int ek_hip_check_sygv_window_xbatched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                             const double *dB, int ldb, long long strideB, const int *m, const double *dw,
                                             const double *dZ, int ldz, int zcap, long long strideZ, const int *info,
                                             double *out, double *ipr, double *seconds);
/* host arrays A, B, w, Z with the same layout (the call works on device copies; the caller's arrays are untouched) */
int ek_hip_check_sygv_window_xbatched(int itype, int n, int batch, const double *A, int lda, long long strideA,
                                      const double *B, int ldb, long long strideB, const int *m, const double *w,
                                      const double *Z, int ldz, int zcap, long long strideZ, const int *info, double *out,
                                      double *ipr, double *seconds);
/* The same for problems of DIFFERENT orders, with the conventions of ek_hip_eigenpairs_vbatched*: n, lda, ldb, ldz, info,
 * out and the pointer arrays dA, dB, dw, dZ, ipr are HOST arrays of `batch` entries; the pointers IN dA, dB, dw, dZ are
 * device addresses (device form) or host addresses (host form), those in ipr always host addresses.
 *   n             : 0 <= n[b] <= EK_HIP_BATCH_NMAX; a problem of order 0 references nothing and gets a_norm = 0 and NaN in
 *                   its other three slots (0 / 0, as the formulas give)
 *   ipr           : NULL, or ipr[b] holds n[b] doubles; a NULL entry means "not wanted for this problem"
 * Return value: -3 n NULL or an order out of range; -4 / -6 / -8 / -9 array NULL or a NULL entry for a problem of order
 * > 0; -5 / -7 / -10 array NULL or a leading dimension below max(1, n[b]); -12 out NULL.  Problem b's outputs are
 * bit-identical to the uniform call's for the same (n, A, B, w, Z). */
int ek_hip_check_vbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                 const double *const *dB, const int *ldb, const double *const *dw,
                                 const double *const *dZ, const int *ldz, const int *info, double *out,
                                 double *const *ipr, double *seconds);
/* host addresses in A, B, w, Z: the lower triangles of A and B travel packed (ld = n[b]), one copy per matrix kind; the
 * caller's arrays are untouched, and a skipped problem's arrays are not read at all */
int ek_hip_check_vbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                          const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                          const int *ldz, const int *info, double *out, double *const *ipr, double *seconds);
/* The variable form for orders up to EK_HIP_XBATCH_NMAX, behind ek_hip_eigenpairs_xvbatched*: what ek_hip_check_xbatched* are
 * to ek_hip_check_batched*, for ek_hip_check_vbatched*.  Prototype for prototype the 14 arguments of
 * ek_hip_check_vbatched_device / ek_hip_check_vbatched, and their whole contract: host arrays of `batch` entries, device
 * (device form) or host (host form) addresses IN dA, dB, dw, dZ, host addresses in ipr (ipr == NULL or a NULL entry: not
 * wanted); A, B, w and Z const and back bit for bit; strictly upper triangles, rows n[b] .. ld-1 and the gaps between
 * problems never read; the same argument-error codes, decided before any device work and without dereferencing any pointer
 * of the pointer arrays, the first offender deciding -- with one difference: -3 is for n == NULL or an order outside
 * 0 .. EK_HIP_XBATCH_NMAX.  n[b] == 0: a_norm = 0 and NaN in the other three slots; info[b] != 0: NaN in the four slots, the
 * ipr row left alone, w and Z not read (host form: nothing of that problem is staged); batch == 0: 0, nothing referenced or
 * written.  ek_hip_check_vbatched* keep answering -3 above EK_HIP_BATCH_NMAX.
 * THE SAME BITS AS THE UNIFORM CALL: problem b's four words and IPRs are those of ek_hip_check_xbatched_device for the same
 * (n, A, B, w, Z) alone -- wherever it sits, whatever surrounds it, in whichever chunk, in the host and the device form (a
 * batch without an order above EK_HIP_BATCH_NMAX returns the bits of ek_hip_check_vbatched*).
 * One stable sort by descending order; the orders above EK_HIP_BATCH_NMAX form a class of their own that runs first, in
 * chunks of at most 1024 checked problems (ek_hip_debug_check_xbatched_chunk governs it), with the kernel of
 * ek_hip_check_xbatched* reading its problem from the table; then the classes of 128, 64 and 32 as in ek_hip_check_vbatched*.
 * Everything runs on one stream: one table upload, the launches, one fetch, one synchronise.  NOT COLLECTIVE.
 * Workspace: that of ek_hip_check_vbatched*; only when an order above EK_HIP_BATCH_NMAX is present, the scratch is at least
 * the largest chunk's sum of n[b]^2 doubles of a generalized batch (at most 512 MiB; the other classes lie over the same
 * buffer). */
int ek_hip_check_xvbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                  const double *const *dB, const int *ldb, const double *const *dw,
                                  const double *const *dZ, const int *ldz, const int *info, double *out,
                                  double *const *ipr, double *seconds);
int ek_hip_check_xvbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                           const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                           const int *ldz, const int *info, double *out, double *const *ipr, double *seconds);

/* The same checks for DSYGV's three problem types -- what ek_hip_check_batched* / ek_hip_check_vbatched* are to
 * ek_hip_eigenpairs_*batched*, these are to ek_hip_sygv_batched* / ek_hip_sygv_vbatched*.  With B = L L^T (B SPD), A and B
 * symmetric by their lower triangles, all n columns checked and plain IEEE divisions:
 *                 type 1 (A x = l B x)          type 2 (A B x = l x)          type 3 (B A x = l x)
 *   r_j           A z_j - w_j B z_j             A (B z_j) - w_j z_j           B (A z_j) - w_j z_j
 *   rho_j         ||r_j||_2 / ||A||_F           ||r_j||_2 / (||A||_F ||B||_F ||z_j||_2)   (types 2 and 3)
 *   G             Z^T B Z                       Z^T B Z                       (L^-1 Z)^T (L^-1 Z)  (= Z^T B^-1 Z)
 *   out[4 b + 0]  the norm the residuals are divided by: ||A||_F (type 1), ||A||_F ||B||_F (types 2 and 3)
 *   out[4 b + 1]  sum_j rho_j / n
 *   out[4 b + 2]  max_j rho_j
 *   out[4 b + 3]  || D^-1/2 G D^-1/2 with zero diagonal ||_F, D = diag(G): scaled by the computed G_jj, as above
 *   ipr           ipr_j = sum_i z_ij^4 / G_jj^2, with the G of the type
 * Type 3 needs a factor of B: the check makes its own from the caller's ORIGINAL B (right-looking Cholesky inside the
 * workgroup).  A pivot that is not positive and finite gives NaN in out[4 b + 3] and in the problem's ipr slots; its
 * residual slots stay valid, and the return value is unaffected.
 * Argument k is argument k of the corresponding ek_hip_check_*batched* entry, itype (1, 2, 3) in the place of problem; B is
 * always required.  Return value: -1 for itype outside 1 .. 3, then the codes of those entries with problem = 1 (uniform:
 * -7 / -8 / -9 for B, ldb, strideB; variable: -6 / -7 for dB, ldb), decided before any device work and without
 * dereferencing a data pointer.  info, out, ipr, seconds, skipped problems, n = 0 and batch = 0 behave as there (NaN in
 * the four slots of a skipped problem, its ipr left alone).
 * itype 1 IS ek_hip_check_*batched*(problem = 1): the same bits in out and ipr.  For the same (B, Z), out[4 b + 3] and ipr
 * of type 2 are the bits of type 1.  THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on (itype, n, A, B,
 * w, Z) alone, in the uniform and the variable form, in the host and the device form.  One launch per call (uniform), at
 * most three (variable), one workgroup per problem, the classes n <= 32 / 64 / 128; A, B, w and Z are const and come back
 * bit for bit; strictly upper triangles, rows n .. ld-1 and the gaps between problems are never read.
 * NOT COLLECTIVE; the calls synchronise.  Workspace: that of ek_hip_check_*batched* for a generalized batch (n^2 doubles
 * per checked problem: S = B Z, then A Z and L in turn). */
int ek_hip_check_sygv_batched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                     const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                     int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                     double *seconds);
int ek_hip_check_sygv_batched(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                              int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                              const int *info, double *out, double *ipr, double *seconds);
/* The uniform form for orders up to EK_HIP_XBATCH_NMAX, behind ek_hip_sygv_xbatched*.  Argument for argument these are
 * ek_hip_check_sygv_batched_device / ek_hip_check_sygv_batched -- 17 arguments, the same argument-error codes decided before
 * any device work and without dereferencing a data pointer, the first offending argument deciding, B always required --
 * with two differences: -1 is for itype outside 1 .. 3 and comes first, -2 is for n < 0 or n > EK_HIP_XBATCH_NMAX.
 *   0 <= n <= EK_HIP_BATCH_NMAX : forwarded to the code behind ek_hip_check_sygv_batched*: the same bits in out and ipr
 *   EK_HIP_BATCH_NMAX < n, itype 1 : ek_hip_check_xbatched*(problem = 1) itself: the same bits
 *   EK_HIP_BATCH_NMAX < n, itype 2, 3 : a kernel class of its own, one workgroup of 512 threads per problem from first load
 *                   to last store.  The quantities are the ones tabulated above, in the same slots.  The three n^3
 *                   products of a type (B Z, A (B Z), Z^T (B Z); A Z, B (A Z), W^T W) run on the fp64 matrix cores over
 *                   LDS-staged tiles with the operands in device memory; type 3's own factor B = L L^T (from the caller's
 *                   ORIGINAL B; a pivot takes a square root and a division) and W = L^-1 Z run in device memory with a
 *                   wave along consecutive rows.  A pivot of B that is not positive and finite gives NaN in out[4 b + 3]
 *                   and in the problem's ipr slots; its residual slots stay valid and the return value is 0
 * The whole contract above holds at the new orders: A and B symmetric by their lower triangles (strictly upper triangles,
 * rows n..ld-1 and the gaps between problems are never read), info = NULL checks every problem and a problem with
 * info[b] != 0 gets NaN in its four slots, keeps its ipr slots and has its w and Z left unread, ipr = NULL is legal,
 * out = NULL is -15, n = 0 or batch = 0 returns 0 with nothing referenced or written, plain IEEE divisions, a maximum that
 * keeps a NaN.  THE SAME BITS WHEREVER A PROBLEM SITS: a problem's outputs depend on (itype, n, A, B, w, Z) alone -- alone,
 * at any position of any batch, in any chunk, in the host and the device form.  For the same (B, Z), out[4 b + 3] and ipr
 * of type 2 are the bits of ek_hip_check_xbatched*(problem = 1).  A, B, w and Z are const and come back bit for bit.
 * NOT COLLECTIVE; the calls synchronise.
 * A batch of types 2 and 3 above EK_HIP_BATCH_NMAX runs in chunks of at most 1024 checked problems (the value that
 * ek_hip_debug_check_xbatched_chunk sets governs this entry too), launched one after the other on one stream without a
 * host synchronise in between; one copy brings the output words to the host, where they are scattered.
 * Workspace there (device memory, grown on demand, kept until ek_hip_finalize): for each of the min(checked problems, 1024)
 * problems of a chunk n^2 doubles for type 2 (S = B Z; at most 512 MiB) and 2 n^2 for type 3 (A Z, then L, and W; at most
 * 1 GiB), 4 + n doubles per problem for the outputs, 4 bytes per checked problem when some are skipped, two events.  All
 * ek_hip_check_*batched* entries draw on ONE such set of buffers, as large as the largest call so far needed.
 * ek_hip_check_sygv_batched* and ek_hip_check_batched* keep answering -2 above EK_HIP_BATCH_NMAX.  The variable-order form
 * above EK_HIP_BATCH_NMAX is ek_hip_check_sygv_xvbatched* below (ek_hip_sygv_xvbatched*' results in one call). */
int ek_hip_check_sygv_xbatched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                      const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                      int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                      double *seconds);
/* host arrays A, B, w, Z with the same layout (the call works on device copies; the caller's arrays are untouched) */
int ek_hip_check_sygv_xbatched(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                               int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                               const int *info, double *out, double *ipr, double *seconds);
/* The variable form of ek_hip_check_sygv_batched* (orders up to EK_HIP_BATCH_NMAX) */
int ek_hip_check_sygv_vbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                      const double *const *dB, const int *ldb, const double *const *dw,
                                      const double *const *dZ, const int *ldz, const int *info, double *out,
                                      double *const *ipr, double *seconds);
int ek_hip_check_sygv_vbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                               const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                               const int *ldz, const int *info, double *out, double *const *ipr, double *seconds);
/* The variable form for orders up to EK_HIP_XBATCH_NMAX, behind ek_hip_sygv_xvbatched*: the 14 arguments and the contract of
 * ek_hip_check_sygv_vbatched*, with -3 for n == NULL or an order outside 0 .. EK_HIP_XBATCH_NMAX (-1 for itype outside 1 .. 3
 * comes first; B always required: -6 / -7).  Problem b's four words and IPRs are the bits of
 * ek_hip_check_sygv_xbatched_device for the same (itype, n, A, B, w, Z) alone, wherever it sits, in whichever chunk, in the
 * host and the device form; itype 1 IS ek_hip_check_xvbatched*(problem = 1); slot 3 and the IPRs of type 2 are type 1's
 * bits; a B that is not SPD under type 3 gives NaN in slot 3 and the IPRs, valid residual slots and the return value 0.
 * Classes, chunks, stream and copies are those of ek_hip_check_xvbatched*, with the kernel of ek_hip_check_sygv_xbatched* in
 * the class above EK_HIP_BATCH_NMAX; its scratch is n[b]^2 doubles per entry of a chunk for type 2 and 2 n[b]^2 for type 3
 * (at most 512 MiB and 1 GiB).  ek_hip_check_sygv_vbatched* keep answering -3 above EK_HIP_BATCH_NMAX.  NOT COLLECTIVE; the
 * calls synchronise once. */
int ek_hip_check_sygv_xvbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                       const double *const *dB, const int *ldb, const double *const *dw,
                                       const double *const *dZ, const int *ldz, const int *info, double *out,
                                       double *const *ipr, double *seconds);
int ek_hip_check_sygv_xvbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                                const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                                const int *ldz, const int *info, double *out, double *const *ipr, double *seconds);
/* The window checks for problems of DIFFERENT orders, behind ek_hip_eigenpairs_window_xvbatched* and
 * ek_hip_sygv_window_xvbatched*: problem b has the c = m[b] values dw[b][0 .. c) and the columns 0 .. c-1 of the
 * n[b] x zcap[b] array dZ[b].  The 14 arguments of ek_hip_check_xvbatched* with m in front of dw and zcap behind ldz, so
 * that the solvers' n, m, dw, dZ, ldz, zcap and info are handed over unchanged.  n, lda, ldb, m, ldz, zcap, info, out and
 * the pointer arrays are HOST arrays of `batch` entries; the pointers IN dA, dB, dw, dZ are device addresses (device form)
 * or host addresses (host form), those in ipr always host addresses (ipr == NULL or a NULL entry: not wanted; ipr[b] holds
 * at least m[b] doubles, m[b] are written).  dA, dB: the ORIGINAL matrices, lower triangles only.
 * Per checked problem, with c = m[b]: exactly the four words and c IPRs that ek_hip_check_window_xbatched* (problem 0 / 1)
 * or ek_hip_check_sygv_window_xbatched* (itype 1 .. 3) define on c columns, type 3's own factor of the caller's B included
 * (a B that is not positive definite: NaN in slot 3 and in the c IPRs only, return value 0).
 * SKIPPED PROBLEMS: info != NULL and info[b] != 0 gives four NaN, leaves the ipr row alone and looks at nothing of that
 * problem's m, w or Z -- -20 included, where m[b] is a count above zcap[b].  EMPTY WINDOWS: m[b] == 0 is handled the same
 * way.  n[b] == 0 forces m[b] == 0, so an order-0 problem is an empty window and gets FOUR NaN -- not the a_norm = 0 of
 * ek_hip_check_xvbatched*.  A batch with nothing to check is filled on the host without the context or a device;
 * batch == 0 returns 0 with nothing referenced or written.
 * Return value: 0, or -k for argument k of the prototype, the first offender deciding, before any device work and without
 * dereferencing any pointer of the pointer arrays (m and info are read):
 *   -1 problem outside 0 / 1 (sygv forms: itype outside 1 .. 3), before everything, batch = 0 included   -2 batch < 0
 *   -3 n NULL or an order outside 0 .. EK_HIP_XBATCH_NMAX
 *   -4 / -5 dA NULL or a NULL entry for an order > 0; lda NULL or below max(1, n[b])
 *   -6 / -7 the same for dB, ldb (problem 1 only; always in the sygv forms, itype = 1 included)
 *   -8 m NULL, or m[b] outside 0 .. n[b] for a problem that info does not skip
 *   -9 dw NULL or a NULL entry for an order > 0
 *   -10 dZ NULL or a NULL entry for an order > 0 with zcap[b] > 0 (NULL is allowed where zcap[b] = 0, as in the solver)
 *   -11 ldz NULL or below max(1, n[b])
 *   -12 zcap NULL, zcap[b] < 0, or zcap[b] < m[b] for a problem that info does not skip
 *   -14 out NULL;   info, ipr, seconds may be NULL;   <= -1000 a HIP runtime error
 * THE SAME BITS AS THE UNIFORM CALL: problem b's four words and m[b] IPRs are bit for bit those of
 * ek_hip_check_window_xbatched_device (ek_hip_check_sygv_window_xbatched_device) on (n[b], A, B, m[b], w, Z) alone --
 * wherever it sits, whatever surrounds it, in whichever launch, in the host and the device form.  So itype = 1 IS
 * ek_hip_check_window_xvbatched*(problem = 1), and type 2's slot 3 and IPRs are type 1's bits.  NEVER READ: w and Z from
 * m[b] on, strictly upper triangles, rows n[b] .. ld-1, the gaps between problems.  NEVER WRITTEN: A, B, w, Z.
 * The window kernels serve every order in one class, so there are no classes here: one stable sort by descending estimated
 * work (n^2 m, plus n^3 / 3 for type 3), one table upload, launches of at most 1024 entries
 * (ek_hip_debug_check_xbatched_chunk governs it) one after the other on one stream, one fetch, one synchronise; *seconds is
 * the device time from before the first launch to after the last.  NOT COLLECTIVE.
 * Workspace (the pool of all ek_hip_check_*batched* entries): the largest chunk's sum of n[b] m[b] doubles (problem 1,
 * type 2) or n[b]^2 + n[b] m[b] (type 3), nothing for problem 0; 4 doubles per problem and m[b] per wanted IPR row; 64
 * bytes per checked problem.  Host form: the lower triangles travel packed (ld = n[b]), one copy per matrix kind, m[b]
 * values of w and m[b] columns of Z per problem; nothing of a skipped or empty problem is staged. */
int ek_hip_check_window_xvbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                         const double *const *dB, const int *ldb, const int *m, const double *const *dw,
                                         const double *const *dZ, const int *ldz, const int *zcap, const int *info,
                                         double *out, double *const *ipr, double *seconds);
int ek_hip_check_window_xvbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                                  const double *const *B, const int *ldb, const int *m, const double *const *w,
                                  const double *const *Z, const int *ldz, const int *zcap, const int *info, double *out,
                                  double *const *ipr, double *seconds);
int ek_hip_check_sygv_window_xvbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                              const double *const *dB, const int *ldb, const int *m,
                                              const double *const *dw, const double *const *dZ, const int *ldz,
                                              const int *zcap, const int *info, double *out, double *const *ipr,
                                              double *seconds);
int ek_hip_check_sygv_window_xvbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                                       const double *const *B, const int *ldb, const int *m, const double *const *w,
                                       const double *const *Z, const int *ldz, const int *zcap, const int *info,
                                       double *out, double *const *ipr, double *seconds);
/* One problem of ANY order: the quantities above for the first n_cols columns of Z (what a window of ek_hip_sygvx*
 * returns; sum_j rho_j / n_cols, G of order n_cols), out[0 .. 3] and ipr_host[0 .. n_cols-1] (host; ipr_host may be NULL).
 * dA, dB: the ORIGINAL column-major matrices (lda, ldb >= max(1, n); lower triangles referenced), dw: n_cols eigenvalues,
 * dZ: n x n_cols (ldz >= max(1, n)).  itype 1 returns what ek_hip_residual_device, ek_hip_orthogonality_device(1, n_cols)
 * and ek_hip_ipratios_device return, bit for bit.  Types 2 and 3 are composed from the products behind those entries and,
 * for type 3, the factorisation and forward solve of ek_hip_potrf / ek_hip_sygst on a copy of B; a B that is not SPD
 * gives NaN in out[3] and ipr_host, valid residual slots and the return value 0.  A, B, w and Z are const and come back
 * bit for bit.  Return value: -k for argument k (-1 itype outside 1 .. 3, -2 n < 0, -3 n_cols outside 0 .. n, -4 / -6 /
 * -8 / -9 NULL, -5 / -7 / -10 leading dimension, -11 out NULL), the first offender deciding, before any device work;
 * n = 0 or n_cols = 0: 0, nothing referenced or written.  NOT COLLECTIVE; the calls synchronise.
 * Workspace (the library's cached device workspace): 2 n^2 + 2 n n_cols + n_cols^2 + 4 n + 3 n_cols doubles, and for
 * type 3 n (n rounded up to 128) for the factor, 128^2 per 128 rows for its diagonal blocks' inverses and 256 max(n
 * rounded up to 128, n_cols) for the triangular solve; the host form adds device copies of A, B, w and Z. */
int ek_hip_check_sygvx_device(int itype, int n, int n_cols, const double *dA, int lda, const double *dB, int ldb,
                              const double *dw, const double *dZ, int ldz, double out[4], double *ipr_host);
int ek_hip_check_sygvx(int itype, int n, int n_cols, const double *A, int lda, const double *B, int ldb, const double *w,
                       const double *Z, int ldz, double out[4], double *ipr_host);

/* Process grids larger than 1x1 (one rank per GPU): replicated-input mode.
 * The reference broadcasts the global sparse matrices to every rank before the solver runs
 * (main.f90:84-86, bcast_sparse_matrix), so every rank can build the full dense A (and B)
 * locally, with no communication.  Each rank then computes the reduction and the
 * tridiagonal eigenproblem redundantly (bitwise identical on every rank: fixed reduction
 * orders, no atomics) and back-transforms / recovers only the eigenvector columns its grid
 * cell owns -- the columns of Z are independent in PDORMTR and PDTRTRS.
 * No data-path collective is needed; a 1 x P grid shards the last two stages P ways.
 *   A, B    : host, full n x n (lda, ldb >= n), same in/out meaning as in ek_hip_solve,
 *             every rank receives the reflectors / the factor L
 *   w       : out: n doubles on every rank (eigenpairs%blacs%values is replicated)
 *   Z_loc   : out: this rank's block-cyclic piece of the N x N eigenvector matrix,
 *             numroc(n, NB, myrow, 0, nprow) x numroc(n_vec, NB, mycol, 0, npcol) entries valid,
 *             layout of setup_distributed_matrix('Eigenvectors', ...) (distribute_matrix.f90:92-148,
 *             solver_scalapack_all.f90:80-81); NB = desc_Z[4] = desc_Z[5]
 *   grid    : nprow x npcol, this rank at (myrow, mycol), row-major ranks (processes.f90:23)
 * info as ek_hip_solve (argument numbering of this prototype). */
int ek_hip_solve_replicated(int problem, int n, int n_vec,
                            double *A, int lda, double *B, int ldb,
                            double *w,
                            double *Z_loc, const int desc_Z[9],
                            int nprow, int npcol, int myrow, int mycol,
                            double *stage_seconds, int n_stages);

/* Distributed INPUTS on grids larger than 1x1 (the reference's own contract: A_loc, B_loc are
 * the block-cyclic pieces setup_distributed_matrix / distribute_global_sparse_matrix produce,
 * distribute_matrix.f90:92-148, 401-422).  The library has no communication layer of its own;
 * the MPI host lends it one: a hook with the semantics of MPI_Allgatherv on doubles over the
 * grid's ranks in row-major order (rank = myrow * npcol + mycol, processes.f90:23).  With the
 * hook registered, ek_hip_solve accepts any nprow x npcol grid: it assembles the full A (and B)
 * on every rank through the hook, continues as ek_hip_solve_replicated, and returns each
 * rank's pieces of Z, of the reflectors (A_loc) and of L (B_loc); the exchange time is
 * reported in stage_seconds[EK_STAGE_GATHER].  Without a hook such grids are refused
 * (info = -11 / -12).  Hook return value: 0 on success (anything else -> info = -999).
 * INTEGRATION.md shows the Fortran bind(C) wrapper around MPI_Allgatherv. */
typedef int (*ek_hip_allgatherv_fn)(const double *send, long long count, double *recv,
                                    const long long *counts, const long long *displs, void *user);
int ek_hip_set_allgatherv(ek_hip_allgatherv_fn fn, void *user);   /* fn = NULL removes the hook */

/* The exchange step alone (pure host code, no GPU involved): M_full (m x n, ldf) <- all ranks'
 * block-cyclic pieces.  info = -998 when no hook is registered. */
int ek_hip_gather_matrix(int m, int n, const double *M_loc, const int desc[9],
                         int nprow, int npcol, int myrow, int mycol,
                         double *M_full, int ldf);

/* The same with A, B resident in this rank's HBM; dZ_loc (ldz_loc >= local rows) receives the
 * local block-cyclic piece for square blocks nb. */
int ek_hip_solve_device_grid(int problem, int n, int n_vec,
                             double *dA, int lda, double *dB, int ldb,
                             double *dw, double *dZ_loc, int ldz_loc,
                             int nb, int nprow, int npcol, int myrow, int mycol,
                             double *stage_seconds, int n_stages);

/* ---- Communicator of the distributed path: one rank per GPU, RCCL over xGMI in
 * place of the BLACS context the reference creates in setup_distribution (processes.f90:42-66).
 * Rank 0 obtains the id (EK_HIP_COMM_ID_BYTES bytes), the host broadcasts it by its own means
 * (MPI_Bcast in a Fortran/MPI host, torch.distributed in the tests) and every rank calls
 * ek_hip_comm_init with its rank in row-major grid order (myrow*npcol + mycol, processes.f90:23).
 * While a communicator is attached, ek_hip_solve_device_grid / ek_hip_solve_replicated /
 * ek_hip_solve on a grid of exactly that many ranks distribute PDSYTRD over the ranks as a 1 x P team of
 * 128-wide column strips (strip S on rank S mod P, whatever the shape of the caller's grid) on top of the
 * column sharding of the eigenvector stages: from order 512 on the dense -> band stage with one broadcast of
 * a panel's reflectors and one ncclAllReduce of A22 V per panel of 64 columns (the band -> tridiagonal stage
 * then runs replicated after one all-gather of the band); below, the one-stage form with one ncclAllReduce of
 * <= 2n+1 doubles per Householder column.  Since round 6 the divide & conquer is distributed below its top merge too (from
 * order 8192 on: the two heights under the top merge in 128-wide strips of the basis array, one ncclAllGather per round of
 * P strips; the secular equation in P runs of roots -- bit for bit the one-GPU result), and on a grid with more than one
 * process ROW the cells of a process column split its eigenvector columns among them and exchange row pieces pairwise
 * at the end (grouped ncclSend / ncclRecv), so every rank back-transforms n_vec / P columns whatever the grid's shape.
 * All exchanges are issued on the library's streams.
 * With a communicator attached ek_hip_solve also takes the reference's own data contract (block-
 * cyclic pieces of A and B in; pieces of Z, of the reflectors and of L out) on that grid WITHOUT the
 * host hook: only the local pieces cross PCIe, the full matrices are assembled in HBM by one
 * all-gather per matrix and the returned pieces are cut out on the device.
 * Collective: every rank of the communicator must make the same calls in the same order
 * (as main.f90:100-104 does).  Returns: -995 no communicator, -996 RCCL error, -997 RCCL not
 * loadable, -994 rank/grid-cell mismatch. */
#define EK_HIP_COMM_ID_BYTES 128
int ek_hip_comm_unique_id(void *id, int bytes);
int ek_hip_comm_init(const void *id, int bytes, int nranks, int rank);
/* The same distributed stages with every exchange routed through the host's allgatherv hook
 * (ek_hip_set_allgatherv, below) instead of RCCL: for an MPI host on a node without an
 * RCCL-capable fabric, and for multi-process tests that share one GPU.  Every exchange drains
 * the stream and crosses PCIe twice -- a compatibility path.  -998 if no hook is registered. */
int ek_hip_comm_attach_host(int nranks, int rank);
int ek_hip_comm_size(void);                     /* 0 when none is attached */
int ek_hip_comm_rank(void);                     /* -1 when none is attached */
int ek_hip_comm_destroy(void);
/* in-place sum over the ranks of a device vector (the collective PDSYTRD issues per column) */
int ek_hip_comm_allreduce_device(double *dbuf, long long count);

/* Stage-level entry points: one per ScaLAPACK call of the reference, host arrays,
 * 1x1 grid descriptors.  They exist so the path can be replaced call by call.  By default ek_hip_sygst and
 * ek_hip_trtrs solve through the 128-block inverses alone; the production form of the solves (the explicit inverses of
 * the 256 x 256 diagonal blocks that the whole-path call registers) is selected by the hook
 * ek_hip_debug_stage_leaves256 of include/ek_hip_debug.h, which is how the stages are tested as the path runs them. */
/* PDPOTRF('L', n, B, 1, 1, desc_B, info)        generalized_to_standard.f90:24 */
int ek_hip_potrf(int n, double *B_loc, const int desc_B[9]);
/* PDSYGST(1, 'L', n, A, 1,1, desc_A, B, 1,1, desc_B, scale, info)   :37 (B holds L) */
int ek_hip_sygst(int n, double *A_loc, const int desc_A[9],
                 const double *L_loc, const int desc_B[9], double *scale);
/* PDSYTRD('L', n, A, 1,1, desc_A, d, e, tau, work, lwork, info)     solver_scalapack_all.f90:59
 * d(n), e(n-1), tau(n-1) are returned replicated (the reference gathers them, :75-78). */
int ek_hip_sytrd(int n, double *A_loc, const int desc_A[9], double *d, double *e, double *tau);
/* PDSYTRD on a 1 x P process grid (column-block-cyclic, 128-wide blocks).  Input: the full matrix
 * (replicated-input mode), output: as ek_hip_sytrd, complete and bit-identical on every rank.
 *   nteam == 0: this process is one rank of the attached communicator;
 *   nteam >= 1: rehearsal of a whole team of nteam ranks inside this process on one GPU (the
 *               exchange is a device kernel); *mismatch = number of doubles in which the ranks'
 *               results (lower triangle of A, d, e, tau) differ from rank 0's (must be 0). */
int ek_hip_sytrd_team(int n, double *A_loc, const int desc_A[9], double *d, double *e, double *tau,
                      int nteam, long long *mismatch);
/* PDPOTRF('L') on a 1 x P grid (128-wide column blocks, right-looking, one broadcast per block
 * column); nteam and *mismatch as in ek_hip_sytrd_team; returns info (first failing pivot, known
 * to every rank). */
int ek_hip_potrf_team(int n, double *B_loc, const int desc_B[9], int nteam, long long *mismatch);
/* PDSYGST(1,'L') on a 1 x P grid: the two triangular solves sharded by columns, one all-gather
 * (grouped ncclBroadcast) in between; nteam as above.  A_loc returns the reduced matrix (whole
 * columns; the lower triangle is the result) assembled from the owners of the 128-wide strips
 * (nteam >= 1), or only this rank's strips with the other columns left as they were (nteam == 0). */
int ek_hip_sygst_team(int n, double *A_loc, const int desc_A[9],
                      const double *L_loc, const int desc_B[9], int nteam);
/* PDSTEDC('I', n, d, e, Z, 1,1, desc_Z, ...)                         :96
 * d in: diagonal, out: eigenvalues ascending; e in: sub-diagonal (destroyed). */
int ek_hip_stedc(int n, double *d, double *e, double *Z_loc, const int desc_Z[9]);
/* PDORMTR('L','L','N', n, ncols, A, 1,1, desc_A, tau, Z, 1,1, desc_Z, ...)   :115 */
int ek_hip_ormtr(int n, int ncols, const double *A_loc, const int desc_A[9], const double *tau,
                 double *Z_loc, const int desc_Z[9]);
/* PDTRTRS('L','T','N', n, nrhs, B, 1,1, desc_B, Z, 1,1, desc_Z, info)  generalized_to_standard.f90:103 */
int ek_hip_trtrs(int n, int nrhs, const double *L_loc, const int desc_B[9],
                 double *Z_loc, const int desc_Z[9]);
/* PDSYGST(ibtype, 'L', n, A, 1,1, desc_A, B, 1,1, desc_B, scale, info) (B holds L): ibtype 1 is ek_hip_sygst,
 * 2 and 3 give A <- L^T A L (lower triangle; the strict upper triangle of L is not read).  info -k for argument k. */
int ek_hip_sygst_ibtype(int ibtype, int n, double *A_loc, const int desc_A[9],
                        const double *L_loc, const int desc_B[9], double *scale);
/* PDTRMM('L','L','N','N', n, nrhs, 1, B, 1,1, desc_B, Z, 1,1, desc_Z): Z <- L Z, the recovery of itype 3 (the strict
 * upper triangle of L is not read).  Argument codes as ek_hip_trtrs. */
int ek_hip_trmm(int n, int nrhs, const double *L_loc, const int desc_B[9], double *Z_loc, const int desc_Z[9]);

/* Building block exposed for the parity tests: C = alpha op(A) op(B) + beta C on the
 * fp64 matrix cores (host arrays; transa/transb: 0 = 'N', 1 = 'T'; lower_only: only
 * tiles touching the lower triangle are updated, as in a SYRK/SYR2K). */
int ek_hip_dgemm(int transa, int transb, int m, int n, int k, double alpha,
                 const double *A, int lda, const double *B, int ldb,
                 double beta, double *C, int ldc, int lower_only);

/* Device-memory helpers for hosts without a HIP runtime binding of their own. */
int ek_hip_malloc(void **dptr, unsigned long long bytes);
int ek_hip_free(void *dptr);
int ek_hip_memcpy_h2d(void *dst, const void *src, unsigned long long bytes);
int ek_hip_memcpy_d2h(void *dst, const void *src, unsigned long long bytes);
int ek_hip_synchronize(void);
/* Fills a device n x n matrix with the synthetic SPD generator of SURVEY.md 8(d)
 * (seed 1 = A, seed 2 = B), so the large bench configurations need no file or PCIe traffic. */
int ek_hip_synth_matrix_device(int n, unsigned long long seed, double *dM, int ldm);

/* Acceptance checks and IPR on the GPU, with the reference's
 * normalisations.  A and B are the ORIGINAL matrices (the reference rebuilds them from the
 * triplets for the check, verifier.f90:122-131); only their lower triangles are referenced,
 * as PDSYMM('L','L') does.
 *   residual      verifier.f90:75-204   A_norm = ||A||_F, res_ave = sum_j||A v_j - l_j B v_j||/A_norm/n_check,
 *                                       res_max = max_j ||.|| / A_norm   (first n_check columns)
 *   orthogonality verifier.f90:233-330  ||D^-1/2 (V^T B V) D^-1/2 - diag||_F over columns index1..index2 (1-based)
 *   ipratios      distribute_matrix.f90:18-78  sum_i v_ij^4 / (sum_i v_ij (S v)_ij)^2, j < n_vec (host output)
 * Divisions are plain IEEE and the maximum keeps a NaN, as in the batched entries: NaN or Inf in w or in a column of Z
 * that a call looks at shows in that call's outputs (a NaN in w[j]: res_ave AND res_max are NaN, the orthogonality and the
 * IPRs are untouched; a zero column j of Z: the orthogonality and ipr[j] are NaN; A = 0: a_norm = 0, Inf or NaN in the
 * residual slots), and the call still returns 0.  Never read: the strictly upper triangles of A and B and their rows
 * n .. ld-1 (A and B are copied to compact symmetric images before any product), w from n_check on, the rows n .. ldz-1
 * of Z, and the columns of Z outside the checked range (j >= n_check; outside index1 .. index2; j >= n_vec).  dB and ldb
 * are not looked at for problem 0.  Every input is const.  Reductions have a fixed order: equal input, equal bits.
 * Argument errors, -k for argument k of the prototype, decided before any device work, the first offender deciding:
 *   residual       -1 problem, -2 n < 0, -3 n_check outside 0 .. n, -4 dA NULL (n > 0), -5 lda < max(1, n), -6 dB NULL and
 *                  -7 ldb < max(1, n) (problem 1 only), -8 dw NULL and -9 dZ NULL (n_check > 0), -10 ldz < max(1, n)
 *   orthogonality  -1 problem, -2 n < 0, -3 index1 outside 1 .. n (so n = 0 gives -3), -4 index2 outside index1 .. n,
 *                  -5 dB NULL and -6 ldb < n (problem 1 only), -7 dZ NULL, -8 ldz < n
 *   ipratios       -1 problem, -2 n < 0, -3 n_vec outside 0 .. n, -4 dB NULL and -5 ldb < max(1, n) (problem 1 only),
 *                  -6 dZ NULL (n_vec > 0), -7 ldz < max(1, n)
 * n = 0 (residual, ipratios) or a count of 0: 0, no output written. */
int ek_hip_residual_device(int problem, int n, int n_check, const double *dA, int lda,
                           const double *dB, int ldb, const double *dw, const double *dZ, int ldz,
                           double *a_norm, double *res_ave, double *res_max);
int ek_hip_orthogonality_device(int problem, int n, int index1, int index2, const double *dB, int ldb,
                                const double *dZ, int ldz, double *orthogonality);
int ek_hip_ipratios_device(int problem, int n, int n_vec, const double *dB, int ldb,
                           const double *dZ, int ldz, double *ipratios_host);
/* Host-array form for the Fortran host: what = 0 residual (out = A_norm, res_ave, res_max; n_cols =
 * n_check), 1 orthogonality (out[0]; index1..index2), 2 IPR (out[0..n_cols-1]). */
int ek_hip_check(int what, int problem, int n, int n_cols, int index1, int index2,
                 const double *A_loc, const int desc_A[9], const double *B_loc, const int desc_B[9],
                 const double *w, const double *Z_loc, const int desc_Z[9], double *out);

/* ---- The reference's own matrix arguments: ek_sparse_mat_t, replicated 1-based triplets (matrix_io.f90:11-15), as
 * eigen_solver and solve_with_general_scalapack receive them (solver_main.f90:22, :65) and as the verifier rebuilds A
 * and B from (verifier.f90:122-131).  A matrix is (nnz, suf, val): suf = the memory of the Fortran suffix(2, nnz), i.e.
 * interleaved (i_k, j_k) pairs, val = value(nnz).  Entry k stands for (i, j) and (j, i); either triangle may appear; of the
 * entries that name the same unordered pair {i, j} the LAST of the list counts, as in the reference's serial pdelset loop
 * (distribute_matrix.f90:411-418).  The library sorts the list into the CSR of the mirrored matrix on the host (counting
 * sort by row, columns ascending), uploads that, and no dense n x n array exists on the host except Z.  A result depends
 * on the set of surviving entries alone: permuting a duplicate-free list changes no bit.  The lists are const.
 * Argument errors, all entries: -k for argument k of the prototype, decided before any device work, the first offender
 * deciding: a negative nnz; with nnz > 0 a NULL suf or an index outside 1 .. n (the suf argument's code) or a NULL val;
 * the counts, index ranges and pointers outside their ranges.  (nnzB, sufB, valB) are not looked at for problem 0.
 * n = 0: 0, nothing referenced.  Non-finite values pass through to the computation.
 *
 * ek_hip_solve_sparse: ek_hip_solve_replicated with A and B built in HBM (zero fill, then both triangles written from
 * the CSR) -- the meaning of problem, n_vec, w, Z_loc, desc_Z, the grid and stage_seconds, the behaviour on a grid with
 * or without a communicator, and the info values are those of ek_hip_solve_replicated, numbered by this prototype (NaN /
 * Inf in A: -6); w and Z_loc are bit-identical to ek_hip_solve_replicated on the mirrored dense matrices at every grid
 * cell.  A and B as reflectors and L are not returned (the reference deallocates them unread).  The CSR build, the
 * upload and the densification are reported in EK_STAGE_COPY. */
int ek_hip_solve_sparse(int problem, int n, int n_vec,
                        long long nnzA, const int *sufA, const double *valA,
                        long long nnzB, const int *sufB, const double *valB,
                        double *w, double *Z_loc, const int desc_Z[9],
                        int nprow, int npcol, int myrow, int mycol,
                        double *stage_seconds, int n_stages);
/* The three acceptance quantities from the triplets in one call, with the normalisations of ek_hip_residual_device,
 * ek_hip_orthogonality_device and ek_hip_ipratios_device:
 *   out[0..2]  a_norm, res_ave, res_max over the first n_check columns     (skipped when n_check = 0)
 *   out[3]     orthogonality over the columns index1 .. index2, 1-based     (skipped when index2 < index1)
 *   ipr_host   n_ipr inverse participation ratios                          (skipped when n_ipr = 0 or ipr_host = NULL)
 * A skipped part leaves its outputs as they were.  dw: n_check eigenvalues, dZ: n x (the largest column a part uses),
 * ldz >= max(1, n), both in device memory.  A V and S = B V are sparse-times-dense products, a pass over the rows each
 * (a thread sums a row's entries in ascending column order; the sums over rows, waves and workgroups have a fixed
 * order; no atomics), ||A||_F comes from the CSR values; only G = V^T S is a GEMM.  For problem 0, out[3] and the IPRs
 * are the bits of ek_hip_orthogonality_device / ek_hip_ipratios_device (the same GEMM call, the same kernels); the rest
 * agrees with the dense entries to rounding.  Divisions are plain IEEE: an empty A gives a_norm = 0 and Inf / NaN in the
 * residual slots.  Repeated calls and permuted duplicate-free lists give the same bits.
 * -9 / -10: dw / dZ NULL where a part needs it, -11 ldz, -12 n_check outside 0 .. n, -13 / -14 index1 < 1 / index2 > n
 * (when index2 >= index1), -15 n_ipr outside 0 .. n, -16 out NULL with a residual or orthogonality part.
 * NOT COLLECTIVE; the calls synchronise; every input is const.  Workspace: the library's cached device workspace; it
 * holds the CSRs, Z^T, for problem 1 S^T and S, G and vectors -- no n x n image of A or B
 * (ek_hip_debug_sparse_check_workspace_bytes of ek_hip_debug.h states the formula). */
int ek_hip_check_sparse_device(int problem, int n,
                               long long nnzA, const int *sufA, const double *valA,
                               long long nnzB, const int *sufB, const double *valB,
                               const double *dw, const double *dZ, int ldz,
                               int n_check, int index1, int index2, int n_ipr,
                               double out[4], double *ipr_host);
/* the same with w and Z host arrays (Z: n x the largest column a part uses, ldz); device copies of them are added */
int ek_hip_check_sparse(int problem, int n,
                        long long nnzA, const int *sufA, const double *valA,
                        long long nnzB, const int *sufB, const double *valB,
                        const double *w, const double *Z, int ldz,
                        int n_check, int index1, int index2, int n_ipr,
                        double out[4], double *ipr_host);
/* The stage alone, for tests and hosts: M (host, n x n, ldm >= n) <- the mirrored dense matrix, densified on the GPU;
 * bit for bit what the reference's loop builds.  What lies between the columns of M (rows n .. ldm-1) is not written. */
int ek_hip_sparse_to_dense(int n, long long nnz, const int *suf, const double *val, double *M, int ldm);

/* Which tridiagonalisation the whole-path calls use is an implementation detail behind the results
 * contract: orders >= 512 (EK_HIP_TWO_STAGE_MIN overrides, 0 = never) go dense -> band -> tridiagonal
 * (two stages, all O(n^3) work on the matrix cores), smaller ones take the one-stage Householder
 * reduction that ek_hip_sytrd exposes with PDSYTRD's own output convention.  With two stages A_loc
 * returns the band and the first stage's R factors instead of PDSYTRD's reflectors (the reference
 * deallocates A without reading it, solver_scalapack_all.f90:19-124).  The library times a one-off
 * placement probe inside the first large one-stage solve (EK_HIP_PLACEMENT=0 turns it off; it prints
 * nothing unless EK_HIP_PLACEMENT_VERBOSE is set).
 * Tuning, profiling and test hooks are declared in ek_hip_debug.h, not here.
 *
 * Run-time switches: every environment variable the library reads (csrc/ek_switch.h is the one reader; INTEGRATION.md 7
 * says more about each).  A set variable counts as atoi() of its text.  once: the first read is kept for the life of
 * the process; each call: read at every use.
 *   name | default | read | meaning
 *   EK_HIP_TWO_STAGE_MIN | 512 | once | order from which two stages tridiagonalise (0: never)
 *   EK_HIP_DIST_MIN_RANKS | 3 | each call | ranks from which the Cholesky factor and the reduction are distributed
 *   EK_HIP_RCCL_LIB | none | each call | text: the RCCL library to load before the usual names
 *   EK_HIP_PIPE_MIN | 2048 | each call | order from which ek_hip_solve stages through its pipeline (0: never)
 *   EK_HIP_PIPE_TRACE | 0 | once and each call | not 0: the pipeline's report (once), 2: with every job (each call)
 *   EK_HIP_PIPE_LOWER | 1 | once | 0: whole matrices cross PCIe both ways
 *   EK_HIP_PIPE_THREADS_OUT | 2 | once | copy threads on the way out
 *   EK_HIP_ALIAS | 1 | each call | 0: always copy the caller's device arrays
 *   EK_HIP_BAND_INPUT | 1 | each call | 0: no short cut for a matrix that is a band already
 *   EK_HIP_PLACEMENT | 1 | once | 0: no placement probe
 *   EK_HIP_PLACEMENT_VERBOSE | unset | each call | set: the probe's timings on stderr
 *   EK_HIP_TEAM_POISON | unset | each call | test aid: NaN into the strips a rehearsed member does not own
 *   EK_SY2SB_PAIR_MIN | 5120 | each call | rows from which dense -> band takes its panels in pairs (0: never)
 *   EK_SY2SB_LOOKAHEAD_MIN | 5120 | once | rows from which the next panel is factored beside the update
 *   EK_SY2SB_DIST_LOOKAHEAD_MIN | 1024 | each call | the same for a team (0: never)
 *   EK_SB2ST_CHASE | 2 | once | 1: band -> tridiagonal by sweeps through memory only
 *   EK_SB2ST_WGS | unset | each call | test aid: sweeps through memory with this many workgroups
 *   EK_SB2ST_JITTER | 0 | each call | test aid: seed of pauses that shake the position kernel's timing
 *   EK_SB2ST_CENSUS_SPINS | 65536 | each call | polls the position kernel's workgroups wait for each other
 *   EK_Q2_NBLK | by order | each call | blocks of sweeps per pass of Q2: 2, 3 or 4 */

#ifdef __cplusplus
}
#endif
#endif /* EK_HIP_H */
