// acg_amd gfx950 (CDNA4 / MI355X) kernels for distributed conjugate gradient.
//
// Hand-written HIP replacing the reference's hipSPARSE/hipBLAS calls and its
// CUDA-era kernels (reference: acg/cg-kernels-hip.hip, acg/halo-kernels-hip.hip,
// acg/cghip.c:463-585).  Contents, in file order:
//   1. deterministic block reductions (partials + finalize; no fp64 atomics:
//      a 3000-block atomicAdd onto one cacheline measured 74 us for a 25 MB
//      dot on this chip, vs ~8 us for this scheme -- the reference's
//      unsafeAtomicAdd dots, cg-kernels-hip.hip:1229-1286, are both slower
//      and non-deterministic),
//   2. sparse operators, chosen per matrix:
//      * CSR vector kernel (4-64 lanes/row) for irregular rows and matO,
//      * SELL-C-64 / sigma-SELL (sliced ELLPACK, slice = one 64-lane wave):
//        one row per lane, vals/cols column-major per slice so every wave
//        load is a contiguous 512 B line set; NT loads + unroll-8 variants,
//      * Block-SELL for dense dof x dof block structure (FEM): one int32
//        index per block, pair-major values (16 B/lane dwordx4 loads),
//   3. fused CG kernels with device-resident scalars (alpha/beta computed
//      in-kernel from the 8-slot slab; the only per-iteration D2H is the
//      8-byte convergence norm): classic fused update + combined finalize,
//      pipelined 6-vector update with BOTH next-iteration dots fused in,
//      and the megafused single-kernel iteration (SpMV + update + dots,
//      double-buffered w, split matA/matO passes for halo overlap),
//   4. on-GPU stencil-operator generation (SELL/BSELL built directly in
//      HBM at write speed; enables the 288 GB-per-GPU Poisson sizing),
//   5. the monolithic device-side CG (whole solve in ONE cooperative
//      launch) with a hand-rolled agent-scope grid barrier (sc1
//      write-through payloads, per-XCD generation lines, parity counters,
//      bounded spins -- cooperative grid.sync measured ~150 us/sync),
//   6. halo pack gather (no unpack exists: ghosts are received in place),
//   7. multiple right-hand sides: SELL / BSELL SpMM over K = 2, 4, 8
//      interleaved vectors (each matrix value and index read once for K
//      products) and the per-column dot / fused update / finalize / daypx
//      kernels of the batched classic CG,
//   8. block CG over the same multivectors: K x K Gram reductions, the
//      fused block update, the Cholesky-QR re-orthonormalisation and the
//      two one-workgroup dense coefficient kernels,
//   9. the host side: dispatch helpers, one launcher per operation, pybind.
//
// The scalar slab layout (fp64 slots) is shared with solvers/hip.py:
#define S_RR 0         // (r,r) current
#define S_PT 1         // (p,t)
#define S_RR_PREV 2    // (r,r) previous
#define S_BNRM2 3      // (b,b)
#define S_GAMMA 4      // pipelined (r,r);  GAMMA,DELTA adjacent => ONE
#define S_DELTA 5      // pipelined (w,r)   2-double allreduce per iteration
#define S_GAMMA_PREV 6
#define S_ALPHA_PREV 7
#define S_NSLOTS 8

// Block-CG state (section 8): one contiguous fp64 tensor of BS_SIZE slots,
// shared with solvers/hip.py and mirrored in ops/torch_ref.py.  Every
// small matrix owns an 8 x 8 row-major region (entry (a, b) at
// base + a*BS_LD + b) whatever the kernel width K is; a width-K kernel
// reads and writes the leading K x K entries only.
#define BS_LD 8
#define BS_M 0         // M = S^T T (mirrored, rows/cols >= kg identity)
#define BS_XI 64       // xi = M^-1
#define BS_XIC 128     // xi C
#define BS_G 192       // G = W^T W (mirrored, rows/cols >= kg identity)
#define BS_ZETA 256    // zeta, upper triangular, G = zeta^T zeta
#define BS_ZINV 320    // zeta^-1, upper triangular
#define BS_C 384       // C: the residual is R = Q C
#define BS_FLAG 448    // sticky breakdown flag: 0 or 1
#define BS_ITER 449    // block iteration at which the flag was set
#define BS_SIZE 456
// block-CG Gram partials: pair p = (a <= b) of block g at p*BLOCK_MAXG + g
#define BLOCK_MAXG 2048
// Cholesky pivot test: breakdown if d_j <= BLOCK_TAU * (diagonal entry)
#define BLOCK_TAU 1e-6

// partials scratch: [0, MAXG) first accumulator, [MAXG, 2*MAXG) second
#define MAXG 16384

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <array>
#include <cstdint>
#include <vector>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace py = pybind11;

#define WAVE 64
#define BLOCK 256

static inline void check_hip(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

static inline long elem_grid(long n, long per_thread = 4) {
    long blocks = (n + (long)BLOCK * per_thread - 1) / ((long)BLOCK * per_thread);
    if (blocks > 4096) blocks = 4096;  // memory-bound: cap + grid-stride (guide §6 G11)
    if (blocks < 1) blocks = 1;
    return blocks;
}

// ---------------------------------------------------------------------------
// block reduction -> one partial per block (deterministic, no atomics)
__device__ __forceinline__ double block_reduce(double v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v += __shfl_down(v, off, WAVE);
    __shared__ double w[BLOCK / WAVE];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
    if (lane == 0) w[wid] = v;
    __syncthreads();
    if (wid == 0) {
        v = (lane < BLOCK / WAVE) ? w[lane] : 0.0;
        #pragma unroll
        for (int off = (BLOCK / WAVE) / 2; off > 0; off >>= 1)
            v += __shfl_down(v, off, WAVE);
    }
    return v;  // valid in thread 0
}

// 0/0-safe coefficient division: once the recursion residual underflows
// to EXACT zero (a converged solve driven past convergence, e.g. a
// fixed-iteration benchmark with rtol=0 -- measured: Queen rr reaches
// 3e-136 after 500 iterations and would hit 0 near ~1200), alpha/beta
// become 0/0 = NaN and poison every vector.  Dividing to 0 instead
// freezes the (already converged) iterate, which is exactly the right
// no-op behaviour.
__device__ __forceinline__ double safe_div(double a, double b) {
    return b != 0.0 ? a / b : 0.0;
}

// sum partials[0..nblocks) into scal[slot] (+= if ACC)
__global__ void __launch_bounds__(BLOCK)
k_reduce_partials(const double* __restrict__ partials, int nblocks,
                  double* scal, int slot, int accumulate) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) v += partials[i];
    v = block_reduce(v);
    if (threadIdx.x == 0) scal[slot] = accumulate ? scal[slot] + v : v;
}

// ---------------------------------------------------------------------------
// CSR SpMV, vector kernel: LANES lanes cooperate on one row (irregular rows,
// matO).  FUSE_DOT: also reduce dot(x, y_contrib) into partials[blockIdx].
// ROWLIST: indirect row ids (rowlist[r]) -- the row-binned hybrid launches
// this kernel once per length bin with bin-appropriate LANES, the MI355X
// answer to the load-balance problem the reference's merge-path SpMV
// solves (cg-kernels-hip.hip:348-1175): per-row work stays proportional
// to row length, no fp64 atomics, fully deterministic.
template <typename ColT, int LANES, bool ACCUM, bool FUSE_DOT, bool ROWLIST = false>
__global__ void __launch_bounds__(BLOCK)
spmv_csr_vector(long nrows, long rowbase,
                const long* __restrict__ rowptr,
                const ColT* __restrict__ colidx,
                const double* __restrict__ vals,
                const double* __restrict__ x,
                double* __restrict__ y,
                double* __restrict__ partials,
                const int* __restrict__ rowlist = nullptr) {
    const int lane = threadIdx.x & (LANES - 1);
    const long group = ((long)blockIdx.x * BLOCK + threadIdx.x) / LANES;
    const long ngroups = (long)gridDim.x * BLOCK / LANES;
    double dacc = 0.0;
    for (long i = group; i < nrows; i += ngroups) {
        const long r = ROWLIST ? (long)rowlist[i] : i;
        const long k0 = rowptr[r], k1 = rowptr[r + 1];
        double sum = 0.0;
        for (long k = k0 + lane; k < k1; k += LANES)
            sum += vals[k] * x[colidx[k]];
        #pragma unroll
        for (int off = LANES / 2; off > 0; off >>= 1)
            sum += __shfl_down(sum, off, LANES);
        if (lane == 0) {
            const long row = rowbase + r;
            if (ACCUM) y[row] += sum; else y[row] = sum;
            if (FUSE_DOT) dacc += x[row] * sum;
        }
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// ---------------------------------------------------------------------------
// SELL-C-64 SpMV: rows grouped in 64-row slices, vals/cols column-major per
// slice (element j of row (s*64+lane) at sellptr[s] + j*64 + lane).  One wave
// per slice: lane = row; every load is a contiguous 64-lane line; per-row sum
// stays in-register (no cross-lane reduce, no pointer walk).
// Variant knobs (bitmask "variant" on the host API, A/B-tested on MI355X):
//   NT : non-temporal loads for vals/cols (streamed exactly once per SpMV;
//        no-allocate keeps the resident x vector from being evicted from
//        L2 by the 4 GB vals/cols stream)
//   SWZ: XCD-aware slice assignment.  The dispatcher places block b on XCD
//        b%8 (guide §1); mapping contiguous slice ranges to one XCD makes
//        each XCD's x working set ~1/8 of x (~4 MB at Queen scale = its L2).
#define SELL_NT 1
#define SELL_SWZ 2
#define SELL_U8 4

template <typename T>
__device__ __forceinline__ T ld_nt(const T* p) { return __builtin_nontemporal_load(p); }

// ValT: storage type of the operator values, double or float.  fp32-stored
// values keep the same element order (vals.to(float32) is the whole pack
// step) and are widened to fp64 on load, which is exact; x, products, row
// sums, y and the fused dot stay fp64.  Matrix stream 12 -> 8 B per entry.
template <typename ColT, bool ACCUM, bool FUSE_DOT, bool NT, bool SWZ, int UNROLL,
          bool PERM = false, typename ValT = double>
__global__ void __launch_bounds__(BLOCK)
k_spmv_sell(long nslices, long nrows, long rowbase,
          const long* __restrict__ sellptr,   // [nslices+1], element offsets
          const ColT* __restrict__ cols,      // padded entries: col of pad = row
          const ValT* __restrict__ vals,      // pad value = 0
          const double* __restrict__ x,
          double* __restrict__ y,
          double* __restrict__ partials,
          const int* __restrict__ perm = nullptr) {  // SELL row -> matrix row (sigma-sorted)
    const int lane = threadIdx.x & (WAVE - 1);
    long blk = blockIdx.x;
    if (SWZ) {
        // bijective XCD remap of the BLOCK index (dispatcher places block b
        // on XCD b%8): XCD k then owns a contiguous slice range, so its x
        // working set is ~1/8 of x and fits the per-XCD 4 MB L2.
        const long nb = gridDim.x, q = nb / 8, rr = nb % 8, xcd = blk % 8;
        blk = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + blk / 8;
    }
    const long wslice = (blk * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double dacc = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long base = sellptr[s];
        const long len = (sellptr[s + 1] - base) >> 6;  // entries per row
        const ValT* __restrict__ v = vals + base + lane;
        const ColT* __restrict__ c = cols + base + lane;
        double sum = 0.0;
        long j = 0;
        for (; j + UNROLL <= len; j += UNROLL) {
            double a[UNROLL], xx[UNROLL];
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                a[u] = (double)(NT ? ld_nt(v + (j + u) * WAVE) : v[(j + u) * WAVE]);
                const ColT ci = NT ? ld_nt(c + (j + u) * WAVE) : c[(j + u) * WAVE];
                xx[u] = x[ci];
            }
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) sum += a[u] * xx[u];
        }
        for (; j < len; ++j) {
            const double a = (double)(NT ? ld_nt(v + j * WAVE) : v[j * WAVE]);
            const ColT ci = NT ? ld_nt(c + j * WAVE) : c[j * WAVE];
            sum += a * x[ci];
        }
        const long row = PERM ? (long)perm[s * WAVE + lane] : s * WAVE + lane;
        if (row < nrows) {
            if (ACCUM) y[rowbase + row] += sum; else y[rowbase + row] = sum;
            if (FUSE_DOT) dacc += x[rowbase + row] * sum;
        }
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// ---------------------------------------------------------------------------
// Block-SELL (BSELL): SELL over BLOCK-rows for matrices with a dense
// dof x dof block structure (FEM/structural problems like Queen_4147:
// 3 dof per mesh node).  One lane = one block-row (node); per block only
// ONE int32 block-column index covers dof*dof values, cutting index
// traffic from 4 B/nnz to 4/dof^2 B/nnz (Queen dof=3: 12 -> 8.44 B/nnz
// total, ~30% less SpMV traffic -- the iteration is at the HBM roofline,
// so bytes are the only lever left).
//
// Layout per 64-node slice s (bptr in block units):
//   bcol[bptr[s] + j*64 + lane]              block-col of node's j-th block
//   bvals: PAIR-major so each lane's value pair (k, k+1) is 16 B
//   contiguous and clang emits dwordx4 loads (16 B/lane = the coalescing
//   sweet spot): element (j,k,lane) at
//     bptr[s]*dof^2 + j*dof^2*64 + bval_off(k, lane)
//   with bval_off = (k/2)*128 + lane*2 + (k&1) for paired k, and the odd
//   tail element (k = dof^2-1 when dof^2 is odd) at (dof^2-1)*64 + lane.
//   fp32-stored values (ValT = float) keep exactly this element order: a
//   lane's pair is then one 8 B load and a dof-3 block 40 B instead of 76.
//   Values widen to fp64 on load (exact); all arithmetic stays fp64.
__device__ __forceinline__ long stencil_col_node(
    int xi, int yi, int zi, int dx, int dy, int dz, int gx, int gy, int gz,
    const long* __restrict__ pb);  // defined with the stencil generators below

template <int D2>
__device__ __forceinline__ long bval_off(int k, int lane) {
    constexpr int EVEN = D2 & ~1;
    return (k < EVEN) ? (long)(k >> 1) * (2 * WAVE) + lane * 2 + (k & 1)
                      : (long)EVEN * WAVE + lane;
}

template <int DOF, bool FUSE_DOT, typename ValT = double>
__global__ void __launch_bounds__(BLOCK)
k_spmv_bsell(long nslices, long nnodes,
             const long* __restrict__ bptr,
             const int* __restrict__ bcol,
             const ValT* __restrict__ bvals,
             const double* __restrict__ x,
             double* __restrict__ y,
             double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double dacc = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;  // blocks per node
        const int* __restrict__ c = bcol + b0 + lane;
        const ValT* __restrict__ v = bvals + b0 * (DOF * DOF);
        double acc[DOF];
        #pragma unroll
        for (int r = 0; r < DOF; ++r) acc[r] = 0.0;
        for (long j = 0; j < blen; ++j) {
            const int cb = ld_nt(c + j * WAVE);
            double xv[DOF];
            #pragma unroll
            for (int cc = 0; cc < DOF; ++cc) xv[cc] = x[(long)cb * DOF + cc];
            const ValT* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
            #pragma unroll
            for (int k = 0; k < DOF * DOF; ++k) {
                const double a = (double)ld_nt(vj + bval_off<DOF * DOF>(k, lane));
                acc[k / DOF] += a * xv[k % DOF];
            }
        }
        const long node = s * WAVE + lane;
        if (node < nnodes) {
            #pragma unroll
            for (int r = 0; r < DOF; ++r) {
                y[node * DOF + r] = acc[r];
                if (FUSE_DOT) dacc += x[node * DOF + r] * acc[r];
            }
        }
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// ---------------------------------------------------------------------------
// Dual SpMV: the operator applied to TWO separate fp64 vectors in one pass
// over the matrix (residual replacement of the pipelined CG: (b - A x, A p),
// then (A r, A t)).  Same layouts, slice-per-wave mapping, non-temporal
// matrix/index loads and padding conventions as k_spmv_sell / k_spmv_bsell;
// every value and index is loaded once and feeds two gathers.
//   y1 = RESID ? b - A x1 : A x1,   y2 = A x2
// FUSE_DOT: per-block partials of (x1,x1) and (y1,x1) over the owned rows in
// the two-half layout of k_pipelined_fused (partials[blk], partials[MAXG+blk]).
// Both columns run the same sequence of fp operations, so x1 == x2 gives
// bitwise y1 == y2 without RESID.  Unroll 4 keeps 8 gathers in flight per
// lane, the same as the single-vector kernel's unroll 8.
__device__ __forceinline__ void spmv2_dots(double g, double d, double* partials) {
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = g;
        partials[MAXG + blockIdx.x] = d;
    }
}

template <typename ColT, bool RESID, bool FUSE_DOT, bool PERM>
__global__ void __launch_bounds__(BLOCK)
k_spmv2_sell(long nslices, long nrows,
             const long* __restrict__ sellptr,
             const ColT* __restrict__ cols,
             const double* __restrict__ vals,
             const double* __restrict__ x1,
             const double* __restrict__ x2,
             const double* __restrict__ b,
             double* __restrict__ y1,
             double* __restrict__ y2,
             double* __restrict__ partials,
             const int* __restrict__ perm) {
    constexpr int UNROLL = 4;
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double g = 0.0, d = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long base = sellptr[s];
        const long len = (sellptr[s + 1] - base) >> 6;  // entries per row
        const double* __restrict__ v = vals + base + lane;
        const ColT* __restrict__ c = cols + base + lane;
        double sum1 = 0.0, sum2 = 0.0;
        long j = 0;
        for (; j + UNROLL <= len; j += UNROLL) {
            double a[UNROLL], xa[UNROLL], xb[UNROLL];
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                a[u] = ld_nt(v + (j + u) * WAVE);
                const ColT ci = ld_nt(c + (j + u) * WAVE);
                xa[u] = x1[ci];
                xb[u] = x2[ci];
            }
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                sum1 += a[u] * xa[u];
                sum2 += a[u] * xb[u];
            }
        }
        for (; j < len; ++j) {
            const double a = ld_nt(v + j * WAVE);
            const ColT ci = ld_nt(c + j * WAVE);
            sum1 += a * x1[ci];
            sum2 += a * x2[ci];
        }
        const long row = PERM ? (long)perm[s * WAVE + lane] : s * WAVE + lane;
        if (row < nrows) {
            const double o1 = RESID ? b[row] - sum1 : sum1;
            y1[row] = o1;
            y2[row] = sum2;
            if (FUSE_DOT) {
                const double xr = x1[row];
                g += xr * xr;
                d += o1 * xr;
            }
        }
    }
    if (FUSE_DOT) spmv2_dots(g, d, partials);
}

template <int DOF, bool RESID, bool FUSE_DOT>
__global__ void __launch_bounds__(BLOCK)
k_spmv2_bsell(long nslices, long nnodes,
              const long* __restrict__ bptr,
              const int* __restrict__ bcol,
              const double* __restrict__ bvals,
              const double* __restrict__ x1,
              const double* __restrict__ x2,
              const double* __restrict__ b,
              double* __restrict__ y1,
              double* __restrict__ y2,
              double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double g = 0.0, d = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;  // blocks per node
        const int* __restrict__ c = bcol + b0 + lane;
        const double* __restrict__ v = bvals + b0 * (DOF * DOF);
        double acc1[DOF], acc2[DOF];
        #pragma unroll
        for (int r = 0; r < DOF; ++r) { acc1[r] = 0.0; acc2[r] = 0.0; }
        for (long j = 0; j < blen; ++j) {
            const int cb = ld_nt(c + j * WAVE);
            double xa[DOF], xb[DOF];
            #pragma unroll
            for (int cc = 0; cc < DOF; ++cc) {
                xa[cc] = x1[(long)cb * DOF + cc];
                xb[cc] = x2[(long)cb * DOF + cc];
            }
            const double* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
            #pragma unroll
            for (int k = 0; k < DOF * DOF; ++k) {
                const double a = ld_nt(vj + bval_off<DOF * DOF>(k, lane));
                acc1[k / DOF] += a * xa[k % DOF];
                acc2[k / DOF] += a * xb[k % DOF];
            }
        }
        const long node = s * WAVE + lane;
        if (node < nnodes) {
            #pragma unroll
            for (int r = 0; r < DOF; ++r) {
                const long row = node * DOF + r;
                const double o1 = RESID ? b[row] - acc1[r] : acc1[r];
                y1[row] = o1;
                y2[row] = acc2[r];
                if (FUSE_DOT) {
                    const double xr = x1[row];
                    g += xr * xr;
                    d += o1 * xr;
                }
            }
        }
    }
    if (FUSE_DOT) spmv2_dots(g, d, partials);
}

// (r,r) and (w,r) partials in exactly the row order and block partition of
// the fused dual SpMV (lane = SELL row or BSELL node, DOF rows in turn, one
// partial pair per block).  The four-SpMV replacement uses it where the dual
// kernels could run, so switching between the two paths changes the number
// of matrix passes and not one bit of gamma / delta.
template <int DOF, bool PERM>
__global__ void __launch_bounds__(BLOCK)
k_dot2_slices(long nslices, long nunits,
              const double* __restrict__ r,
              const double* __restrict__ w,
              const int* __restrict__ perm,
              double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double g = 0.0, d = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long unit = PERM ? (long)perm[s * WAVE + lane] : s * WAVE + lane;
        if (unit < nunits) {
            #pragma unroll
            for (int k = 0; k < DOF; ++k) {
                const double xr = r[unit * DOF + k];
                const double o1 = w[unit * DOF + k];
                g += xr * xr;
                d += o1 * xr;
            }
        }
    }
    spmv2_dots(g, d, partials);
}

// Tile-symmetric Block-SELL (BSELL-ST): a symmetric operator stores a block
// pair (A_ij, A_ji = A_ij^T) ONCE when both nodes belong to the same
// 256-node tile (= one workgroup).  The owner lane accumulates A x[c] for
// itself and hands A^T x_self to the partner through LDS slot
// lds[q][c - tile_base]; every (slot, node) cell has at most one writer
// (builder invariant), and after one barrier each lane adds its nrecv
// slots in slot order -- no LDS or global atomics, bitwise reproducible.
// Layout per 64-node slice s (sptr in block units, values pair-major as
// in BSELL): blocks j < spl[s] are plain for every lane; blocks
// j >= spl[s] carry a byte sq (slot number, ST_NOSEND = plain or padding).
// x and y are in the builder's permuted node order.  Occupancy is set by
// LDS (qmax 8, dof 3: 48 KiB -> 3 workgroups per CU); unroll 2 keeps two
// blocks' loads in flight per wave, unroll 4 (160 VGPRs) measured the same.
#define ST_NOSEND 255

template <int DOF, bool FUSE_DOT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_bsell_st(long ntiles, long nslices, long nnodes,
                const long* __restrict__ sptr,
                const int* __restrict__ spl,
                const int* __restrict__ scol,
                const unsigned char* __restrict__ sq,
                const double* __restrict__ svals,
                const unsigned char* __restrict__ nrecv,
                const double* __restrict__ x,
                double* __restrict__ y,
                double* __restrict__ partials) {
    extern __shared__ double st_lds[];  // [qmax][DOF][BLOCK]
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
    double dacc = 0.0;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long tile_base = t * BLOCK;
        const long s = t * (BLOCK / WAVE) + wid;
        const long node = tile_base + threadIdx.x;
        const bool live = s < nslices;  // wave-uniform
        double acc[DOF];
        #pragma unroll
        for (int r = 0; r < DOF; ++r) acc[r] = 0.0;
        if (live) {
            const long nself = node < nnodes ? node : nnodes - 1;
            double xs[DOF];
            #pragma unroll
            for (int r = 0; r < DOF; ++r) xs[r] = x[nself * DOF + r];
            const long b0 = sptr[s];
            const long blen = (sptr[s + 1] - b0) >> 6;
            const long npl = spl[s];
            const int* __restrict__ c = scol + b0 + lane;
            const unsigned char* __restrict__ qp = sq + b0 + lane;
            const double* __restrict__ v = svals + b0 * (DOF * DOF);
            #pragma unroll 2
            for (long j = 0; j < npl; ++j) {
                const int cb = ld_nt(c + j * WAVE);
                double xv[DOF];
                #pragma unroll
                for (int cc = 0; cc < DOF; ++cc) xv[cc] = x[(long)cb * DOF + cc];
                const double* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
                #pragma unroll
                for (int k = 0; k < DOF * DOF; ++k) {
                    const double a = ld_nt(vj + bval_off<DOF * DOF>(k, lane));
                    acc[k / DOF] += a * xv[k % DOF];
                }
            }
            #pragma unroll 2
            for (long j = npl; j < blen; ++j) {
                const int cb = ld_nt(c + j * WAVE);
                const int q = ld_nt(qp + j * WAVE);
                double xv[DOF], tr[DOF];
                #pragma unroll
                for (int cc = 0; cc < DOF; ++cc) {
                    xv[cc] = x[(long)cb * DOF + cc];
                    tr[cc] = 0.0;
                }
                const double* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
                #pragma unroll
                for (int k = 0; k < DOF * DOF; ++k) {
                    const double a = ld_nt(vj + bval_off<DOF * DOF>(k, lane));
                    acc[k / DOF] += a * xv[k % DOF];
                    tr[k % DOF] += a * xs[k / DOF];
                }
                if (q != ST_NOSEND) {
                    const int loc = (int)((long)cb - tile_base);
                    #pragma unroll
                    for (int cc = 0; cc < DOF; ++cc)
                        st_lds[(q * DOF + cc) * BLOCK + loc] = tr[cc];
                }
            }
        }
        __syncthreads();
        if (live && node < nnodes) {
            const int nr = nrecv[node];
            for (int q = 0; q < nr; ++q) {
                #pragma unroll
                for (int r = 0; r < DOF; ++r)
                    acc[r] += st_lds[(q * DOF + r) * BLOCK + threadIdx.x];
            }
            #pragma unroll
            for (int r = 0; r < DOF; ++r) {
                y[node * DOF + r] = acc[r];
                if (FUSE_DOT) dacc += x[node * DOF + r] * acc[r];
            }
        }
        __syncthreads();  // the next trip rewrites the slots
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// Classic-CG daypx folded into the BSELL SpMV (serial matA-only path):
// instead of a separate p = beta p + r kernel (3n streams) the gather
// computes beta*p_old[c] + r[c] on the fly and the row side materialises
// p_new = beta*p_old + r into a SEPARATE buffer (ping-pong: folding into
// one buffer would be a write-after-read race against other blocks'
// gathers -- the separate daypx kernel's global barrier is exactly what
// a single buffer needs).  beta = rr/rr_prev from the device scalar
// slab (the previous update's finalize); the host seeds rr_prev = inf
// before iteration 0 so beta = 0 reproduces p0 = r0.  The fused (p,t)
// dot uses the in-register p_new row values.
template <int DOF>
__global__ void __launch_bounds__(BLOCK)
k_spmv_bsell_daypx(long nslices, long nnodes,
                   const long* __restrict__ bptr,
                   const int* __restrict__ bcol,
                   const double* __restrict__ bvals,
                   const double* __restrict__ pold,
                   const double* __restrict__ rvec,
                   double* __restrict__ pnew,
                   double* __restrict__ y,
                   const double* __restrict__ scal,
                   double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    const double beta = safe_div(scal[S_RR], scal[S_RR_PREV]);
    double dacc = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;
        const int* __restrict__ c = bcol + b0 + lane;
        const double* __restrict__ v = bvals + b0 * (DOF * DOF);
        double acc[DOF];
        #pragma unroll
        for (int r = 0; r < DOF; ++r) acc[r] = 0.0;
        for (long j = 0; j < blen; ++j) {
            const int cb = ld_nt(c + j * WAVE);
            double xv[DOF];
            #pragma unroll
            for (int cc = 0; cc < DOF; ++cc)
                xv[cc] = beta * pold[(long)cb * DOF + cc]
                         + rvec[(long)cb * DOF + cc];
            const double* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
            #pragma unroll
            for (int k = 0; k < DOF * DOF; ++k) {
                const double a = ld_nt(vj + bval_off<DOF * DOF>(k, lane));
                acc[k / DOF] += a * xv[k % DOF];
            }
        }
        const long node = s * WAVE + lane;
        if (node < nnodes) {
            #pragma unroll
            for (int r = 0; r < DOF; ++r) {
                const double pn = beta * pold[node * DOF + r]
                                  + rvec[node * DOF + r];
                pnew[node * DOF + r] = pn;
                y[node * DOF + r] = acc[r];
                dacc += pn * acc[r];
            }
        }
    }
    dacc = block_reduce(dacc);
    if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
}

// device-side BSELL generation for the block-stencil slab (block-level
// analog of k_stencil_rowlen / k_stencil_fill; matA only -- owned x owned)
__global__ void __launch_bounds__(BLOCK)
k_stencil_blocklen(long nnodes, int gx, int gy, int gz, long nown_nodes,
                   const int* __restrict__ zs_of_plane,
                   const long* __restrict__ pb,
                   const double* __restrict__ offs, int ksten,
                   long* __restrict__ blocklen) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nnodes; i += stride) {
        const int pl = (int)(i / plane_nodes);
        const long rem = i - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        long cnt = 1;  // self block
        for (int o = 0; o < ksten; ++o) {
            const long cn = stencil_col_node(xi, yi, zi, (int)offs[o * 4],
                                             (int)offs[o * 4 + 1],
                                             (int)offs[o * 4 + 2], gx, gy, gz, pb);
            if (cn >= 0 && cn < nown_nodes) ++cnt;
        }
        blocklen[i] = cnt;
    }
}

template <int DOF>
__global__ void __launch_bounds__(BLOCK)
k_stencil_bfill(long nnodes, int gx, int gy, int gz, long nown_nodes,
                const int* __restrict__ zs_of_plane,
                const long* __restrict__ pb,
                const double* __restrict__ offs, int ksten,
                const double* __restrict__ blocks,  // M then D
                const long* __restrict__ bptr,
                int* __restrict__ bcol, double* __restrict__ bvals) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    const double* M = blocks;
    const double* D = blocks + DOF * DOF;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nnodes; i += stride) {
        const int pl = (int)(i / plane_nodes);
        const long rem = i - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        const long s = i >> 6;
        const int lane = (int)(i & 63);
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;
        long j = 0;
        double* __restrict__ bv = bvals + b0 * DOF * DOF;
        // self block (D)
        bcol[b0 + j * WAVE + lane] = (int)i;
        for (int k = 0; k < DOF * DOF; ++k)
            bv[j * DOF * DOF * WAVE + bval_off<DOF * DOF>(k, lane)] = D[k];
        ++j;
        for (int o = 0; o < ksten; ++o) {
            const long cn = stencil_col_node(xi, yi, zi, (int)offs[o * 4],
                                             (int)offs[o * 4 + 1],
                                             (int)offs[o * 4 + 2], gx, gy, gz, pb);
            if (cn < 0 || cn >= nown_nodes) continue;
            const double w = offs[o * 4 + 3];
            bcol[b0 + j * WAVE + lane] = (int)cn;
            for (int k = 0; k < DOF * DOF; ++k)
                bv[j * DOF * DOF * WAVE + bval_off<DOF * DOF>(k, lane)] = w * M[k];
            ++j;
        }
        for (; j < blen; ++j) {  // padding: self col, zero block
            bcol[b0 + j * WAVE + lane] = (int)i;
            for (int k = 0; k < DOF * DOF; ++k)
                bv[j * DOF * DOF * WAVE + bval_off<DOF * DOF>(k, lane)] = 0.0;
        }
    }
}

// ---------------------------------------------------------------------------
// BLAS-1 / fused CG kernels.  Scalar coefficients come from the device slab.

__global__ void __launch_bounds__(BLOCK)
k_zero_scalars(double* scal, int i0, int count) {
    for (int i = threadIdx.x; i < count; i += BLOCK) scal[i0 + i] = 0.0;
}

// before the classic halo/SpMV: zero the (p,t) accumulator (only needed
// on the CSR fallback path; the SELL/BSELL matA finalize overwrites)
__global__ void k_cg_prep_pt(double* scal) { if (threadIdx.x == 0) scal[S_PT] = 0.0; }

// after allreduce(p,t): save rr for the device-side alpha
__global__ void k_cg_prep_rr(double* scal) {
    if (threadIdx.x == 0) scal[S_RR_PREV] = scal[S_RR];
}

// classic-iteration epilogue: rotate rr -> rr_prev, then publish the new
// (r,r) from the update kernel's partials (one 1-block launch instead of
// prep_rr + reduce_partials)
__global__ void __launch_bounds__(BLOCK)
k_cg_finalize(const double* __restrict__ partials, int nblocks, double* scal) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) v += partials[i];
    v = block_reduce(v);
    if (threadIdx.x == 0) {
        scal[S_RR_PREV] = scal[S_RR];
        scal[S_RR] = v;
    }
}

// Jacobi-PCG fused iteration epilogue (beyond reference -- aCG has no
// preconditioning): alpha = rz/(p,t) from the device slab, then ONE pass
// computes r -= alpha t, x += alpha p, z = dinv .* r, and BOTH next
// scalars rz' = (r,z) and rr' = (r,r).  Replaces axpy_ratio x2 + mul +
// prep + dot x2 (6 launches, ~13n traffic) with 1 launch + a finalize.
__global__ void __launch_bounds__(BLOCK)
k_pcg_fused_update(double* __restrict__ r, double* __restrict__ x,
                   const double* __restrict__ p, const double* __restrict__ t,
                   double* __restrict__ z, const double* __restrict__ dinv,
                   long n, const double* __restrict__ scal,
                   double* __restrict__ partials) {
    const double alpha = safe_div(scal[S_RR], scal[S_PT]);  // S_RR = rz
    double arz = 0.0, arr = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double rn = r[i] - alpha * ld_nt(t + i);
        r[i] = rn;
        __builtin_nontemporal_store(ld_nt(x + i) + alpha * p[i], x + i);
        const double zi = dinv[i] * rn;
        z[i] = zi;
        arz += rn * zi;
        arr += rn * rn;
    }
    arz = block_reduce(arz);
    __syncthreads();  // block_reduce reuses its LDS scratch
    arr = block_reduce(arr);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = arz;
        partials[MAXG + blockIdx.x] = arr;
    }
}

// finalize: rotate rz -> rz_prev (S_RR -> S_RR_PREV), publish rz' in
// S_RR and the true rr' in S_GAMMA
__global__ void __launch_bounds__(BLOCK)
k_pcg_finalize(const double* __restrict__ partials, int nblocks,
               double* scal) {
    double vz = 0.0, vr = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
        vz += partials[i];
        vr += partials[MAXG + i];
    }
    vz = block_reduce(vz);
    __syncthreads();
    vr = block_reduce(vr);
    if (threadIdx.x == 0) {
        scal[S_RR_PREV] = scal[S_RR];
        scal[S_RR] = vz;
        scal[S_GAMMA] = vr;
    }
}

// ---------------------------------------------------------------------------
// Block-Jacobi PCG on Block-SELL operators (beyond reference, opt-in):
// M = blockdiag(A_node,node), the dof x dof diagonal block of every node.
// The inverse blocks are symmetric and stored as their packed upper
// triangle, NC = dof(dof+1)/2 doubles per node, row-major over (a <= b),
// laid out [slice][component][64]: component c of lane's node sits at
//   (s*NC + c)*64 + lane
// so every component is one contiguous 512 B wave load.  One lane per node
// throughout (the mapping of k_spmv_bsell); r/t/x/p/z are touched at
// stride dof per lane like that kernel's y write.
__host__ __device__ constexpr int bj_tri(int a, int b, int dof) {
    // packed-upper index of (a, b), a <= b
    return a * dof - a * (a - 1) / 2 + (b - a);
}

// setup: sum every block of the node's list whose bcol is the node itself
// (the self block plus any zero-valued padding blocks -- both packers pad
// short nodes with zero blocks that name the node, k_stencil_bfill after
// the real blocks and bsell_from_csr wherever the node's list ends, so a
// sum is right under either and does not depend on block order), factor
// it M = L L^T and store M^-1 = L^-T L^-1.  A node without a diagonal
// block, or with a pivot that is <= 0 or not finite, counts into *status
// (integer atomic: order-independent) and gets a zero inverse.  Lanes past
// nnodes in the last slice do nothing.  Always reads the fp64 bvals.
template <int DOF>
__global__ void __launch_bounds__(BLOCK)
k_bsell_diag_inv(long nslices, long nnodes,
                 const long* __restrict__ bptr,
                 const int* __restrict__ bcol,
                 const double* __restrict__ bvals,
                 double* __restrict__ minv,
                 int* __restrict__ status) {
    constexpr int D2 = DOF * DOF;
    constexpr int NC = DOF * (DOF + 1) / 2;
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    for (long s = wslice; s < nslices; s += nw) {
        const long node = s * WAVE + lane;
        if (node >= nnodes) continue;
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;
        const int* __restrict__ c = bcol + b0 + lane;
        const double* __restrict__ v = bvals + b0 * D2;
        double d[D2];
        #pragma unroll
        for (int k = 0; k < D2; ++k) d[k] = 0.0;
        int found = 0;
        for (long j = 0; j < blen; ++j) {
            if ((long)c[j * WAVE] != node) continue;
            ++found;
            const double* __restrict__ vj = v + j * D2 * WAVE;
            #pragma unroll
            for (int k = 0; k < D2; ++k) d[k] += vj[bval_off<D2>(k, lane)];
        }
        // Cholesky of the lower triangle
        bool ok = found > 0;
        double l[DOF][DOF];
        #pragma unroll
        for (int j = 0; j < DOF; ++j) {
            double piv = d[j * DOF + j];
            #pragma unroll
            for (int q = 0; q < j; ++q) piv -= l[j][q] * l[j][q];
            ok = ok && piv > 0.0 && piv <= 1.79769313486231570815e308;
            const double ljj = sqrt(piv);
            l[j][j] = ljj;
            #pragma unroll
            for (int i = j + 1; i < DOF; ++i) {
                double t = d[i * DOF + j];
                #pragma unroll
                for (int q = 0; q < j; ++q) t -= l[i][q] * l[j][q];
                l[i][j] = t / ljj;
            }
        }
        // li = L^-1 (lower triangular), column by column
        double li[DOF][DOF];
        #pragma unroll
        for (int cc = 0; cc < DOF; ++cc) {
            #pragma unroll
            for (int i = cc; i < DOF; ++i) {
                double t = (i == cc) ? 1.0 : 0.0;
                #pragma unroll
                for (int q = cc; q < i; ++q) t -= l[i][q] * li[q][cc];
                li[i][cc] = t / l[i][i];
            }
        }
        // M^-1(a, b) = sum_{k >= b} li[k][a] * li[k][b],  a <= b
        double* __restrict__ out = minv + s * (NC * WAVE) + lane;
        #pragma unroll
        for (int a = 0; a < DOF; ++a) {
            #pragma unroll
            for (int b = a; b < DOF; ++b) {
                double t = 0.0;
                #pragma unroll
                for (int k = b; k < DOF; ++k) t += li[k][a] * li[k][b];
                out[bj_tri(a, b, DOF) * WAVE] = ok ? t : 0.0;
            }
        }
        if (!ok) atomicAdd(status, 1);
    }
}

template <int DOF>
__device__ __forceinline__ void bj_load_inv(const double* __restrict__ minv,
                                            long node,
                                            double (&m)[DOF * (DOF + 1) / 2]) {
    constexpr int NC = DOF * (DOF + 1) / 2;
    const double* __restrict__ q = minv + (node >> 6) * (NC * WAVE) + (node & (WAVE - 1));
    #pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = q[c * WAVE];
}

// z = M^-1_node r  (row a: sum over b in ascending order)
template <int DOF>
__device__ __forceinline__ void bj_mul(const double (&m)[DOF * (DOF + 1) / 2],
                                       const double (&r)[DOF], double (&z)[DOF]) {
    #pragma unroll
    for (int a = 0; a < DOF; ++a) {
        double acc = 0.0;
        #pragma unroll
        for (int b = 0; b < DOF; ++b)
            acc += m[a <= b ? bj_tri(a, b, DOF) : bj_tri(b, a, DOF)] * r[b];
        z[a] = acc;
    }
}

// z = M^-1 r with the partials of (r,z) and (r,r) in the two halves of
// the scratch (k_pcg_finalize's layout): z0 of the block-Jacobi PCG
template <int DOF>
__global__ void __launch_bounds__(BLOCK)
k_bjacobi_apply(const double* __restrict__ minv, const double* __restrict__ r,
                double* __restrict__ z, long nnodes,
                double* __restrict__ partials) {
    double arz = 0.0, arr = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nnodes; i += stride) {
        double rv[DOF], zv[DOF], m[DOF * (DOF + 1) / 2];
        #pragma unroll
        for (int a = 0; a < DOF; ++a) rv[a] = r[i * DOF + a];
        bj_load_inv<DOF>(minv, i, m);
        bj_mul<DOF>(m, rv, zv);
        #pragma unroll
        for (int a = 0; a < DOF; ++a) {
            z[i * DOF + a] = zv[a];
            arz += rv[a] * zv[a];
            arr += rv[a] * rv[a];
        }
    }
    arz = block_reduce(arz);
    __syncthreads();  // block_reduce reuses its LDS scratch
    arr = block_reduce(arr);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = arz;
        partials[MAXG + blockIdx.x] = arr;
    }
}

// block form of k_pcg_fused_update: alpha = rz/(p,t) from the device slab,
// r -= alpha t, x += alpha p, z_node = M^-1_node r'_node from the new r in
// registers, partials of rz' and rr'.  Same non-temporal choices: t and x
// are single-use, r/z/p stay cacheable.  Traffic: 7n vector doubles plus
// (dof+1)/2 n of packed inverse (9n for dof 3 against point Jacobi's 8n).
template <int DOF>
__global__ void __launch_bounds__(BLOCK)
k_bpcg_fused_update(double* __restrict__ r, double* __restrict__ x,
                    const double* __restrict__ p, const double* __restrict__ t,
                    double* __restrict__ z, const double* __restrict__ minv,
                    long nnodes, const double* __restrict__ scal,
                    double* __restrict__ partials) {
    const double alpha = safe_div(scal[S_RR], scal[S_PT]);  // S_RR = rz
    double arz = 0.0, arr = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nnodes; i += stride) {
        double rn[DOF], zv[DOF], m[DOF * (DOF + 1) / 2];
        #pragma unroll
        for (int a = 0; a < DOF; ++a) {
            const long e = i * DOF + a;
            rn[a] = r[e] - alpha * ld_nt(t + e);
            r[e] = rn[a];
            __builtin_nontemporal_store(ld_nt(x + e) + alpha * p[e], x + e);
        }
        bj_load_inv<DOF>(minv, i, m);
        bj_mul<DOF>(m, rn, zv);
        #pragma unroll
        for (int a = 0; a < DOF; ++a) {
            z[i * DOF + a] = zv[a];
            arz += rn[a] * zv[a];
            arr += rn[a] * rn[a];
        }
    }
    arz = block_reduce(arz);
    __syncthreads();  // block_reduce reuses its LDS scratch
    arr = block_reduce(arr);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = arz;
        partials[MAXG + blockIdx.x] = arr;
    }
}

// dot: partials[b] = block sum of x[i]*y[i]
__global__ void __launch_bounds__(BLOCK)
k_dot(const double* __restrict__ x, const double* __restrict__ y, long n,
      double* __restrict__ partials) {
    double acc = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        acc += x[i] * y[i];
    acc = block_reduce(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// fused dot2 (pipelined init): gamma_b = sum r*r, delta_b = sum w*r
__global__ void __launch_bounds__(BLOCK)
k_dot2(const double* __restrict__ r, const double* __restrict__ w, long n,
       double* __restrict__ partials) {
    double g = 0.0, d = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double ri = r[i];
        g += ri * ri;
        d += w[i] * ri;
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = g;
        partials[MAXG + blockIdx.x] = d;
    }
}

// sum both dot2 partial sets into scal[GAMMA], scal[DELTA]
__global__ void __launch_bounds__(BLOCK)
k_reduce_partials2(const double* __restrict__ partials, int nblocks,
                   double* scal, int accumulate) {
    double g = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
        g += partials[i];
        d += partials[MAXG + i];
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        scal[S_GAMMA] = accumulate ? scal[S_GAMMA] + g : g;
        scal[S_DELTA] = accumulate ? scal[S_DELTA] + d : d;
    }
}

// y += sign * (scal[num]/scal[den]) * x
__global__ void __launch_bounds__(BLOCK)
k_axpy_ratio(double* __restrict__ y, const double* __restrict__ x, long n,
             const double* __restrict__ scal, int num, int den, double sign) {
    const double a = sign * safe_div(scal[num], scal[den]);
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        y[i] += a * x[i];
}

// y = (scal[num]/scal[den]) * y + x      (daypx with device beta)
__global__ void __launch_bounds__(BLOCK)
k_daypx_ratio(double* __restrict__ y, const double* __restrict__ x, long n,
              const double* __restrict__ scal, int num, int den) {
    const double b = safe_div(scal[num], scal[den]);
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        y[i] = b * y[i] + x[i];
}

// classic-CG fused update: alpha = rr/pt (device; S_RR still holds the
// current rr -- k_cg_finalize rotates it afterwards);
//   r -= alpha*t;  x += alpha*p;  partials[b] = block sum of new r.r
// One pass over r,t,x,p instead of three kernels + a dot
// (reference: daxpy_minus_alpha + daxpy_alpha + Ddot, cghip.c:969-1026).
__global__ void __launch_bounds__(BLOCK)
k_cg_fused_update(double* __restrict__ r, double* __restrict__ x,
                  const double* __restrict__ p, const double* __restrict__ t,
                  long n, const double* __restrict__ scal,
                  double* __restrict__ partials) {
    const double alpha = safe_div(scal[S_RR], scal[S_PT]);
    double acc = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    // t and x are single-use streams this iteration: non-temporal keeps
    // p (the next SpMV's gather source) and r resident in L2/L3
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double rn = r[i] - alpha * ld_nt(t + i);
        r[i] = rn;
        __builtin_nontemporal_store(ld_nt(x + i) + alpha * p[i], x + i);
        acc += rn * rn;
    }
    acc = block_reduce(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__device__ __forceinline__ void pipelined_coeffs(const double* scal, int first,
                                                 double* beta, double* alpha) {
    const double gamma = scal[S_GAMMA], delta = scal[S_DELTA];
    if (first) { *beta = 0.0; *alpha = safe_div(gamma, delta); }
    else {
        const double b = safe_div(gamma, scal[S_GAMMA_PREV]);
        *beta = b;
        *alpha = safe_div(gamma,
                          delta - b * safe_div(gamma, scal[S_ALPHA_PREV]));
    }
}

// pipelined-CG fused 6-vector update (Ghysels-Vanroose), device scalars,
// WITH the next iteration's dots fused in: after updating r,w this kernel
// already holds the new values in registers, so gamma' = (r',r') and
// delta' = (w',r') cost zero extra memory traffic.  The separate dot2 pass
// of the reference (two hipblasDdot, cghip.c:1735-1752) disappears from
// the iteration.
template <bool NTU>
__global__ void __launch_bounds__(BLOCK)
k_pipelined_fused(double* __restrict__ z, double* __restrict__ t,
                  double* __restrict__ p, double* __restrict__ x,
                  double* __restrict__ r, double* __restrict__ w,
                  const double* __restrict__ q, long n,
                  const double* __restrict__ scal, int first,
                  double* __restrict__ partials) {
    double beta, alpha;
    pipelined_coeffs(scal, first, &beta, &alpha);
    double g = 0.0, d = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    // NTU: z,t,p,x,q are touched once per iteration -- non-temporal so
    // their ~400 MB/iter of streams do not evict w (the next SpMV's
    // gather source) or r from L2/L3.
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const double zi = (NTU ? ld_nt(q + i) : q[i]) + beta * (NTU ? ld_nt(z + i) : z[i]);
        const double ti = w[i] + beta * (NTU ? ld_nt(t + i) : t[i]);
        const double pi = r[i] + beta * (NTU ? ld_nt(p + i) : p[i]);
        const double xn = (NTU ? ld_nt(x + i) : x[i]) + alpha * pi;
        if (NTU) {
            __builtin_nontemporal_store(zi, z + i);
            __builtin_nontemporal_store(ti, t + i);
            __builtin_nontemporal_store(pi, p + i);
            __builtin_nontemporal_store(xn, x + i);
        } else {
            z[i] = zi; t[i] = ti; p[i] = pi; x[i] = xn;
        }
        const double rn = r[i] - alpha * ti;
        const double wn = w[i] - alpha * zi;
        r[i] = rn; w[i] = wn;
        g += rn * rn;
        d += wn * rn;
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = g;
        partials[MAXG + blockIdx.x] = d;
    }
}

// ---------------------------------------------------------------------------
// MEGAFUSED pipelined-CG iteration: SELL SpMV with the entire Ghysels-
// Vanroose 6-vector update + both next-iteration dots fused into the SpMV
// epilogue.  Requires a double-buffered w (the SpMV gathers w_old while the
// epilogue writes w_new), which makes the per-row update race-free: every
// other stream (z,t,p,x,r) is touched only at the row's own index.
// The whole iteration becomes ONE kernel (+ a 1-block finalize), and the
// intermediate q vector disappears entirely (never stored, never re-read):
// per-iteration HBM traffic drops from SELL + 15n doubles to SELL + 11n.
//
// Split-SpMV distribution support: the matA pass (MATO=false) fully updates
// interior rows (no ghost couplings) and defers border rows by storing
// their partial q into qpart; the matO pass (MATO=true) adds the ghost
// contributions, reads qpart, and updates the border rows -- so the halo
// exchange still overlaps the matA pass exactly like the reference's split
// (cghip.c:887-931).
template <typename ColT, bool NT, int UNROLL, bool MATO>
__global__ void __launch_bounds__(BLOCK)
k_sell_pipe(long nslices, long nrows_pass, long rowbase, long border_base,
            const long* __restrict__ sellptr, const ColT* __restrict__ cols,
            const double* __restrict__ vals,
            const double* __restrict__ w_old,  // gather source (nlocal)
            double* __restrict__ qpart,        // border q staging [nowned-border_base]
            double* __restrict__ z, double* __restrict__ t,
            double* __restrict__ p, double* __restrict__ x,
            double* __restrict__ r, double* __restrict__ w_new,
            const double* __restrict__ scal, int first,
            double* __restrict__ partials, long partials_off) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double beta, alpha;
    pipelined_coeffs(scal, first, &beta, &alpha);
    double g = 0.0, d = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long base = sellptr[s];
        const long len = (sellptr[s + 1] - base) >> 6;
        const double* __restrict__ v = vals + base + lane;
        const ColT* __restrict__ c = cols + base + lane;
        double sum = 0.0;
        long j = 0;
        for (; j + UNROLL <= len; j += UNROLL) {
            double a[UNROLL], xx[UNROLL];
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                a[u] = NT ? ld_nt(v + (j + u) * WAVE) : v[(j + u) * WAVE];
                xx[u] = w_old[c[(j + u) * WAVE]];
            }
            #pragma unroll
            for (int u = 0; u < UNROLL; ++u) sum += a[u] * xx[u];
        }
        for (; j < len; ++j)
            sum += (NT ? ld_nt(v + j * WAVE) : v[j * WAVE]) * w_old[c[j * WAVE]];
        const long rr = s * WAVE + lane;
        if (rr < nrows_pass) {
            const long row = rowbase + rr;
            if (!MATO && row >= border_base) {
                qpart[row - border_base] = sum;  // defer to the matO pass
            } else {
                const double q = MATO ? sum + qpart[row - border_base] : sum;
                const double zi = q + beta * ld_nt(z + row);
                const double ti = w_old[row] + beta * ld_nt(t + row);
                const double pi = r[row] + beta * ld_nt(p + row);
                __builtin_nontemporal_store(zi, z + row);
                __builtin_nontemporal_store(ti, t + row);
                __builtin_nontemporal_store(pi, p + row);
                __builtin_nontemporal_store(ld_nt(x + row) + alpha * pi, x + row);
                const double rn = r[row] - alpha * ti;
                const double wn = w_old[row] - alpha * zi;
                r[row] = rn; w_new[row] = wn;
                g += rn * rn;
                d += wn * rn;
            }
        }
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[partials_off + blockIdx.x] = g;
        partials[MAXG + partials_off + blockIdx.x] = d;
    }
}

// one-block epilogue of a pipelined iteration: persist gamma_prev/alpha_prev
// from the OLD gamma/delta, then overwrite gamma/delta with the freshly
// reduced sums from k_pipelined_fused's partials.
__global__ void __launch_bounds__(BLOCK)
k_pipelined_finalize(const double* __restrict__ partials, int nblocks,
                     double* scal, int first) {
    double g = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
        g += partials[i];
        d += partials[MAXG + i];
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        double beta, alpha;
        pipelined_coeffs(scal, first, &beta, &alpha);
        scal[S_GAMMA_PREV] = scal[S_GAMMA];
        scal[S_ALPHA_PREV] = alpha;
        scal[S_GAMMA] = g;
        scal[S_DELTA] = d;
    }
}

// Finalize of a residual replacement: gamma = (r,r) and delta = (w,r) of the
// recomputed vectors, from the partials of the fused dual SpMV.  Writes ONLY
// S_GAMMA and S_DELTA: k_pipelined_finalize of the iteration just finished
// has already rotated S_GAMMA_PREV / S_ALPHA_PREV.
__global__ void __launch_bounds__(BLOCK)
k_pipelined_replace_finalize(const double* __restrict__ partials, int nblocks,
                             double* scal) {
    double g = 0.0, d = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
        g += partials[i];
        d += partials[MAXG + i];
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        scal[S_GAMMA] = g;
        scal[S_DELTA] = d;
    }
}

// ---------------------------------------------------------------------------
// Device-side stencil-operator generation: build the slab-local SELL arrays
// for a block-stencil SPD operator directly in HBM.  The operator is
// analytic (offsets + dof x dof blocks), so there is no reason to assemble
// 100+ GB of CSR on the host and copy it over PCIe: a 2048^3 7-pt Poisson
// slab (~90 GB of SELL data per GPU) generates in well under a second at
// HBM write speed, sized for the 288 GB of HBM3E per GPU.
// Mirrors acg_amd/gen/stencil.py::stencil_local_slab (same plane ordering:
// interior | border | ghost, ghosts sorted by (owner, global id)); column
// order within a row is enumeration order (SpMV needs no sorted columns).
//
// pb: plane z (+1 shift) -> local node base, -1 if absent  (int64[gz+2])
// offs: ksten stencil offsets as (dx, dy, dz, w) doubles
// zs_of_plane: local plane index -> z                      (int32[nplanes])
// blocks: M (offblock) then D (diagblock), dof*dof doubles each
// filter_ghost: 0 = keep cols with local node < nown_nodes (matA),
//               1 = keep ghost cols only (matO; row range given by rowbase)

__device__ __forceinline__ long stencil_col_node(
    int xi, int yi, int zi, int dx, int dy, int dz, int gx, int gy, int gz,
    const long* __restrict__ pb) {
    const int nx = xi + dx, ny = yi + dy, nz = zi + dz;
    if (nx < 0 || nx >= gx || ny < 0 || ny >= gy || nz < 0 || nz >= gz)
        return -1;
    const long base = pb[nz + 1];
    if (base < 0) return -1;
    return base + nx + (long)gx * ny;
}

__global__ void __launch_bounds__(BLOCK)
k_stencil_rowlen(long nrows_nodes, long row0_node, int gx, int gy, int gz,
                 int dof, long nown_nodes,
                 const int* __restrict__ zs_of_plane,
                 const long* __restrict__ pb,
                 const double* __restrict__ offs, int ksten,
                 int filter_ghost, long* __restrict__ rowlen) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nrows_nodes;
         i += stride) {
        const long node = row0_node + i;
        const int pl = (int)(node / plane_nodes);
        const long rem = node - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        long cnt = filter_ghost ? 0 : 1;  // self is always owned
        for (int o = 0; o < ksten; ++o) {
            const int dx = (int)offs[o * 4 + 0], dy = (int)offs[o * 4 + 1],
                      dz = (int)offs[o * 4 + 2];
            const long cn = stencil_col_node(xi, yi, zi, dx, dy, dz, gx, gy, gz, pb);
            if (cn < 0) continue;
            const bool ghost = cn >= nown_nodes;
            if (ghost == (bool)filter_ghost) ++cnt;
        }
        rowlen[i] = cnt * dof;  // every (node,a) row has the same length
    }
}

__global__ void __launch_bounds__(BLOCK)
k_stencil_fill(long nrows_nodes, long row0_node, int gx, int gy, int gz,
               int dof, long nown_nodes,
               const int* __restrict__ zs_of_plane,
               const long* __restrict__ pb,
               const double* __restrict__ offs, int ksten,
               const double* __restrict__ blocks,  // M then D, dof*dof each
               int filter_ghost,
               const long* __restrict__ sellptr,
               int* __restrict__ cols, double* __restrict__ vals) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    const double* M = blocks;
    const double* D = blocks + dof * dof;
    const long nrows = nrows_nodes * dof;
    for (long row = (long)blockIdx.x * BLOCK + threadIdx.x; row < nrows;
         row += stride) {
        const long nodei = row / dof;
        const int a = (int)(row - nodei * dof);
        const long node = row0_node + nodei;
        const int pl = (int)(node / plane_nodes);
        const long rem = node - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        const long s = row >> 6;
        const int lane = (int)(row & 63);
        const long base = sellptr[s];
        const long len = (sellptr[s + 1] - base) >> 6;
        long j = 0;
        if (!filter_ghost) {  // self block first
            for (int bb = 0; bb < dof; ++bb, ++j) {
                cols[base + j * WAVE + lane] = (int)(node * dof + bb);
                vals[base + j * WAVE + lane] = D[a * dof + bb];
            }
        }
        for (int o = 0; o < ksten; ++o) {
            const int dx = (int)offs[o * 4 + 0], dy = (int)offs[o * 4 + 1],
                      dz = (int)offs[o * 4 + 2];
            const double w = offs[o * 4 + 3];
            const long cn = stencil_col_node(xi, yi, zi, dx, dy, dz, gx, gy, gz, pb);
            if (cn < 0) continue;
            const bool ghost = cn >= nown_nodes;
            if (ghost != (bool)filter_ghost) continue;
            for (int bb = 0; bb < dof; ++bb, ++j) {
                cols[base + j * WAVE + lane] = (int)(cn * dof + bb);
                vals[base + j * WAVE + lane] = w * M[a * dof + bb];
            }
        }
        // pad to slice length: self column, zero value
        const int selfcol = (int)(filter_ghost ? 0 : node * dof + a);
        for (; j < len; ++j) {
            cols[base + j * WAVE + lane] = selfcol;
            vals[base + j * WAVE + lane] = 0.0;
        }
    }
}

// ---------------------------------------------------------------------------
// MATRIX-FREE stencil operator (dof=1, constant coefficients -- 5/7/27-pt
// Poisson-type).  The assembled operator re-reads 12 B/nnz of vals+cols per
// SpMV that the stencil makes redundant: y[i] = diag*x[i] + sum w*x[nb] is
// fully determined by the grid coordinates.  Applying it matrix-free reads
// ONLY x (largely L2-cached across the 7/27 neighbour touches) and writes y,
// dropping per-iteration HBM traffic by the whole vals+cols stream -- and
// removes the operator from HBM entirely (a 2048^3 7-pt slab is ~90 GB of
// SELL; matrix-free it is 0).  Beyond the reference (aCG always assembles);
// opt-in because real matrices (Queen_4147) have position-dependent values
// and MUST be measured with the memory-resident operator.
//
// Same matA/matO split as the assembled path: the matA pass covers owned
// couplings (diag included), the matO pass adds ghost-plane couplings to
// border rows after the halo lands.
template <bool MATO, bool FUSE_DOT>
__global__ void __launch_bounds__(BLOCK)
k_stencil_spmv(long nrows_nodes, long row0_node, int gx, int gy, int gz,
               long nown_nodes,
               const int* __restrict__ zs_of_plane,
               const long* __restrict__ pb,
               const double* __restrict__ offs, int ksten, double diag,
               const double* __restrict__ x, double* __restrict__ y,
               double* __restrict__ partials) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    double dacc = 0.0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nrows_nodes;
         i += stride) {
        const long node = row0_node + i;
        const int pl = (int)(node / plane_nodes);
        const long rem = node - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        double sum = MATO ? 0.0 : diag * x[node];
        for (int o = 0; o < ksten; ++o) {
            const int dx = (int)offs[o * 4 + 0], dy = (int)offs[o * 4 + 1],
                      dz = (int)offs[o * 4 + 2];
            const long cn = stencil_col_node(xi, yi, zi, dx, dy, dz,
                                             gx, gy, gz, pb);
            if (cn < 0) continue;
            if ((cn >= nown_nodes) == MATO) sum += offs[o * 4 + 3] * x[cn];
        }
        if (MATO) y[node] += sum; else y[node] = sum;
        if (FUSE_DOT) dacc += x[node] * sum;
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// Megafused matrix-free pipelined iteration: identical epilogue and qpart /
// partials protocol to k_sell_pipe (see there), with the SpMV computed from
// the stencil instead of SELL loads.  Per-iteration traffic collapses to
// the 11n-double vector stream alone.
template <bool MATO>
__global__ void __launch_bounds__(BLOCK)
k_stencil_pipe(long nrows_nodes, long row0_node, long border_base,
               int gx, int gy, int gz, long nown_nodes,
               const int* __restrict__ zs_of_plane,
               const long* __restrict__ pb,
               const double* __restrict__ offs, int ksten, double diag,
               const double* __restrict__ w_old, double* __restrict__ qpart,
               double* __restrict__ z, double* __restrict__ t,
               double* __restrict__ p, double* __restrict__ xv,
               double* __restrict__ r, double* __restrict__ w_new,
               const double* __restrict__ scal, int first,
               double* __restrict__ partials, long partials_off) {
    const long stride = (long)gridDim.x * BLOCK;
    const long plane_nodes = (long)gx * gy;
    double beta, alpha;
    pipelined_coeffs(scal, first, &beta, &alpha);
    double g = 0.0, d = 0.0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nrows_nodes;
         i += stride) {
        const long node = row0_node + i;
        const int pl = (int)(node / plane_nodes);
        const long rem = node - (long)pl * plane_nodes;
        const int xi = (int)(rem % gx), yi = (int)(rem / gx);
        const int zi = zs_of_plane[pl];
        double sum = MATO ? 0.0 : diag * w_old[node];
        for (int o = 0; o < ksten; ++o) {
            const int dx = (int)offs[o * 4 + 0], dy = (int)offs[o * 4 + 1],
                      dz = (int)offs[o * 4 + 2];
            const long cn = stencil_col_node(xi, yi, zi, dx, dy, dz,
                                             gx, gy, gz, pb);
            if (cn < 0) continue;
            if ((cn >= nown_nodes) == MATO) sum += offs[o * 4 + 3] * w_old[cn];
        }
        const long row = node;  // dof = 1
        if (!MATO && row >= border_base) {
            qpart[row - border_base] = sum;  // defer to the matO pass
        } else {
            const double q = MATO ? sum + qpart[row - border_base] : sum;
            const double zi_ = q + beta * ld_nt(z + row);
            const double ti = w_old[row] + beta * ld_nt(t + row);
            const double pi = r[row] + beta * ld_nt(p + row);
            __builtin_nontemporal_store(zi_, z + row);
            __builtin_nontemporal_store(ti, t + row);
            __builtin_nontemporal_store(pi, p + row);
            __builtin_nontemporal_store(ld_nt(xv + row) + alpha * pi, xv + row);
            const double rn = r[row] - alpha * ti;
            const double wn = w_old[row] - alpha * zi_;
            r[row] = rn; w_new[row] = wn;
            g += rn * rn;
            d += wn * rn;
        }
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[partials_off + blockIdx.x] = g;
        partials[MAXG + partials_off + blockIdx.x] = d;
    }
}

// 7-pt z-column-walk specialisation: one thread owns one (x,y) column and
// walks the owned planes z0..z1-1, carrying the z-1/z/z+1 values of w_old
// in registers.  The generic kernel re-reads the z +- 1 planes through an
// L2 that cannot hold them (a 512^2 plane is 2 MB x thousands of in-flight
// blocks), costing ~2 extra w_old streams; the walk reads w_old EXACTLY
// once.  x +- 1 / y +- gx neighbours come from L1 (adjacent lanes load
// them).  matA pass only -- ghost-plane couplings stay with the generic
// matO kernel (2 planes at most).
template <bool FUSE_DOT>
__global__ void __launch_bounds__(BLOCK)
k_stencil_spmv7(long plane_nodes, int gx, int z0, int z1, int gz,
                long nown_nodes, const long* __restrict__ pb,
                double diag, double wxm, double wxp, double wym, double wyp,
                double wzm, double wzp,
                const double* __restrict__ x, double* __restrict__ y,
                double* __restrict__ partials) {
    const long stride = (long)gridDim.x * BLOCK;
    double dacc = 0.0;
    for (long xy = (long)blockIdx.x * BLOCK + threadIdx.x; xy < plane_nodes;
         xy += stride) {
        const int xi = (int)(xy % gx);
        const long yi = xy / gx;
        const bool hxm = xi > 0, hxp = xi < gx - 1;
        const bool hym = yi > 0, hyp = yi < plane_nodes / gx - 1;
        long base_c = pb[z0 + 1];
        double xc = x[base_c + xy];
        const long base_m = (z0 > 0) ? pb[z0] : -1;
        bool hm = base_m >= 0 && base_m < nown_nodes;
        double xm = hm ? x[base_m + xy] : 0.0;
        for (int zz = z0; zz < z1; ++zz) {
            const long node = base_c + xy;
            const long base_p = (zz + 1 < gz) ? pb[zz + 2] : -1;
            const bool hp = base_p >= 0 && base_p < nown_nodes;
            const double xp = hp ? x[base_p + xy] : 0.0;
            double sum = diag * xc;
            if (hxm) sum += wxm * x[node - 1];
            if (hxp) sum += wxp * x[node + 1];
            if (hym) sum += wym * x[node - gx];
            if (hyp) sum += wyp * x[node + gx];
            if (hm) sum += wzm * xm;
            if (hp) sum += wzp * xp;
            y[node] = sum;
            if (FUSE_DOT) dacc += xc * sum;
            xm = xc; hm = true;
            xc = xp; base_c = base_p;
        }
    }
    if (FUSE_DOT) {
        dacc = block_reduce(dacc);
        if (threadIdx.x == 0) partials[blockIdx.x] = dacc;
    }
}

// megafused 7-pt column walk: k_stencil_pipe's epilogue on the walk above.
__global__ void __launch_bounds__(BLOCK)
k_stencil_pipe7(long plane_nodes, int gx, int z0, int z1, int gz,
                long border_base, long nown_nodes,
                const long* __restrict__ pb,
                double diag, double wxm, double wxp, double wym, double wyp,
                double wzm, double wzp,
                const double* __restrict__ w_old, double* __restrict__ qpart,
                double* __restrict__ z, double* __restrict__ t,
                double* __restrict__ p, double* __restrict__ xv,
                double* __restrict__ r, double* __restrict__ w_new,
                const double* __restrict__ scal, int first,
                double* __restrict__ partials, long partials_off) {
    const long stride = (long)gridDim.x * BLOCK;
    double beta, alpha;
    pipelined_coeffs(scal, first, &beta, &alpha);
    double g = 0.0, d = 0.0;
    for (long xy = (long)blockIdx.x * BLOCK + threadIdx.x; xy < plane_nodes;
         xy += stride) {
        const int xi = (int)(xy % gx);
        const long yi = xy / gx;
        const bool hxm = xi > 0, hxp = xi < gx - 1;
        const bool hym = yi > 0, hyp = yi < plane_nodes / gx - 1;
        long base_c = pb[z0 + 1];
        double xc = w_old[base_c + xy];
        const long base_m = (z0 > 0) ? pb[z0] : -1;
        bool hm = base_m >= 0 && base_m < nown_nodes;
        double xm = hm ? w_old[base_m + xy] : 0.0;
        for (int zz = z0; zz < z1; ++zz) {
            const long node = base_c + xy;
            const long base_p = (zz + 1 < gz) ? pb[zz + 2] : -1;
            const bool hp = base_p >= 0 && base_p < nown_nodes;
            const double xp = hp ? w_old[base_p + xy] : 0.0;
            double sum = diag * xc;
            if (hxm) sum += wxm * w_old[node - 1];
            if (hxp) sum += wxp * w_old[node + 1];
            if (hym) sum += wym * w_old[node - gx];
            if (hyp) sum += wyp * w_old[node + gx];
            if (hm) sum += wzm * xm;
            if (hp) sum += wzp * xp;
            if (node >= border_base) {
                qpart[node - border_base] = sum;  // matO finishes border rows
            } else {
                const double zi_ = sum + beta * ld_nt(z + node);
                const double ti = xc + beta * ld_nt(t + node);
                const double pi = r[node] + beta * ld_nt(p + node);
                __builtin_nontemporal_store(zi_, z + node);
                __builtin_nontemporal_store(ti, t + node);
                __builtin_nontemporal_store(pi, p + node);
                __builtin_nontemporal_store(ld_nt(xv + node) + alpha * pi,
                                            xv + node);
                const double rn = r[node] - alpha * ti;
                const double wn = xc - alpha * zi_;
                r[node] = rn; w_new[node] = wn;
                g += rn * rn;
                d += wn * rn;
            }
            xm = xc; hm = true;
            xc = xp; base_c = base_p;
        }
    }
    g = block_reduce(g);
    __syncthreads();
    d = block_reduce(d);
    if (threadIdx.x == 0) {
        partials[partials_off + blockIdx.x] = g;
        partials[MAXG + partials_off + blockIdx.x] = d;
    }
}

// ---------------------------------------------------------------------------
// Monolithic device-side CG: the ENTIRE solver loop in one cooperative
// launch -- zero per-iteration launch/sync overhead (reference
// acgsolverhip_cg_kernel, cg-kernels-hip.hip:1386-1747; single-GPU, like
// the reference's HIP build).  MI355X design: SELL-C-64 SpMV, grid-wide
// barriers via cooperative groups, per-block partials reduced by block 0
// (deterministic).  Residency: the launcher sizes the grid from the
// occupancy query, everything inside is grid-stride.
#include <hip/hip_cooperative_groups.h>

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
typedef __attribute__((address_space(1))) unsigned int gu32;

// Hand-rolled grid barrier (guide §6 G16): cooperative_groups::grid.sync()
// measured ~150 us per sync on ROCm 7.2.  v2 design, after measuring a
// per-block release-fence + single-word-poll version still slow at >1000
// blocks:
//  - ALL shared payloads (vectors, partials) are written WRITE-THROUGH
//    (sc1: relaxed agent-scope 8-byte atomic stores) so no release fence
//    (no per-block buffer_wbl2 storm) is needed -- every wave just drains
//    vmcnt before its block arrives (guide R1 + pitfall 14).
//  - waiters poll a PER-XCD copy of the generation word (the dispatcher
//    places block b on XCD b%8, so each poll line serves ~1/8 of the
//    blocks; correctness does not depend on the placement, every copy is
//    written).  Polling is RELAXED with s_sleep backoff; ONE acquire
//    (L1 invalidate) per block after wake.  Spins are bounded: on timeout
//    fail[0] is set and every block exits (no hang).
// barrier_state layout (u32 words): [0]=cnt(even phases), [8]=cnt(odd
// phases) (sense-reversing parity counters: the releaser resets the
// just-used counter, which no block touches again until two barriers
// later -- a racing early arrival for the NEXT barrier targets the OTHER
// word, so the reset can never eat an arrival), [1]=fail,
// [16+16*x]=generation copy for XCD x (64 B stride: distinct lines).
#define BAR_GEN0 16
#define BAR_GENSTRIDE 16
// hierarchical-barrier extension words (v3): per-XCD arrival counters on
// distinct cachelines, one set per parity: [144+16x] even, [272+16x] odd.
#define BAR_XCNT0 144
#define BAR_XCNT_PAR 128
#define BAR_STATE_WORDS 400

__device__ __forceinline__ void st_sc1_f64(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p),
                       (unsigned long long)__double_as_longlong(v), RLX_AGENT);
}

// Hierarchical barrier (v3): arrivals first bump a PER-XCD counter line
// (blocks land on XCD b%8, so the ~128 RMWs per line proceed on 8 lines
// in parallel instead of 1024 serialised on one line -- the ~35 us cost
// of the flat barrier at 1024 blocks); each XCD's last arriver bumps the
// global counter (<= 8 RMWs); the global last resets BOTH levels of the
// current parity and bumps every generation copy.  Parity safety is the
// same argument as the flat barrier: the words being reset belong to the
// phase that no block will touch again until two barriers later.
__device__ __forceinline__ bool grid_barrier_hier(unsigned* state) {
    gu32* fail = (gu32*)(state + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    bool ok = true;
    if (threadIdx.x == 0) {
        const int myxcd = (int)(blockIdx.x & 7);
        const unsigned nb = gridDim.x;
        const unsigned q = nb >> 3, rmd = nb & 7u;
        const unsigned blocks_on_mine = q + ((unsigned)myxcd < rmd ? 1u : 0u);
        const unsigned nxcd = nb < 8u ? nb : 8u;
        gu32* mygen = (gu32*)(state + BAR_GEN0 + BAR_GENSTRIDE * myxcd);
        const unsigned g = __hip_atomic_load(mygen, RLX_AGENT);
        const unsigned par = g & 1u;
        gu32* xcnt = (gu32*)(state + BAR_XCNT0 + BAR_XCNT_PAR * par
                             + BAR_GENSTRIDE * myxcd);
        const unsigned ax = __hip_atomic_fetch_add(xcnt, 1u, RLX_AGENT) + 1u;
        bool releaser = false;
        if (ax == blocks_on_mine) {
            gu32* gcnt = (gu32*)(state + (par ? 8 : 0));
            const unsigned ag = __hip_atomic_fetch_add(gcnt, 1u, RLX_AGENT) + 1u;
            if (ag == nxcd) {
                __hip_atomic_store(gcnt, 0u, RLX_AGENT);
                #pragma unroll
                for (int xx = 0; xx < 8; ++xx)
                    __hip_atomic_store(
                        (gu32*)(state + BAR_XCNT0 + BAR_XCNT_PAR * par
                                + BAR_GENSTRIDE * xx), 0u, RLX_AGENT);
                #pragma unroll
                for (int xx = 0; xx < 8; ++xx)
                    __hip_atomic_store(
                        (gu32*)(state + BAR_GEN0 + BAR_GENSTRIDE * xx),
                        g + 1u, RLX_AGENT);
                releaser = true;
            }
        }
        if (!releaser) {
            unsigned spins = 0;
            while (__hip_atomic_load(mygen, RLX_AGENT) == g) {
                if (spins < 32) __builtin_amdgcn_s_sleep(2);
                else __builtin_amdgcn_s_sleep(64);
                if (++spins > 4000000u) {
                    __hip_atomic_store(fail, 1u, RLX_AGENT);
                    ok = false;
                    break;
                }
                if (__hip_atomic_load(fail, RLX_AGENT)) { ok = false; break; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return ok;
}

__device__ __forceinline__ bool grid_barrier(unsigned* state) {
    gu32* fail = (gu32*)(state + 1);
    // every wave: drain pending sc1 payload stores before signalling (also
    // completes this block's own reset/gen stores from the previous
    // barrier before its new arrival -- the parity-counter safety hinges
    // on this drain)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    bool ok = true;
    if (threadIdx.x == 0) {
        const int myxcd = (int)(blockIdx.x & 7);
        gu32* mygen = (gu32*)(state + BAR_GEN0 + BAR_GENSTRIDE * myxcd);
        const unsigned g = __hip_atomic_load(mygen, RLX_AGENT);
        gu32* cnt = (gu32*)(state + ((g & 1u) ? 8 : 0));
        const unsigned arrived = __hip_atomic_fetch_add(cnt, 1u, RLX_AGENT) + 1u;
        if (arrived == gridDim.x) {
            __hip_atomic_store(cnt, 0u, RLX_AGENT);
            #pragma unroll
            for (int xx = 0; xx < 8; ++xx)
                __hip_atomic_store((gu32*)(state + BAR_GEN0 + BAR_GENSTRIDE * xx),
                                   g + 1u, RLX_AGENT);
        } else {
            unsigned spins = 0;
            while (__hip_atomic_load(mygen, RLX_AGENT) == g) {
                if (spins < 32) __builtin_amdgcn_s_sleep(2);
                else __builtin_amdgcn_s_sleep(64);
                if (++spins > 4000000u) {  // ~7 s worst case: fail fast, never hang
                    __hip_atomic_store(fail, 1u, RLX_AGENT);
                    ok = false;
                    break;
                }
                if (__hip_atomic_load(fail, RLX_AGENT)) { ok = false; break; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return ok;
}

// results: scal[S_BNRM2]=(b,b), scal[S_RR_PREV]=(r0,r0), scal[S_RR]=final
// (r,r); out2[0]=niterations, out2[1]=converged (-1 = barrier timeout).
// barrier_state: 3 zeroed u32 words {cnt, gen, fail}.
template <typename ColT>
__global__ void __launch_bounds__(BLOCK)
k_cg_device(long nslices, long nrows,
            const long* __restrict__ sellptr, const ColT* __restrict__ cols,
            const double* __restrict__ vals,
            const double* __restrict__ b, double* __restrict__ x,
            double* __restrict__ r, double* __restrict__ p,
            double* __restrict__ t,
            double* __restrict__ scal, double* __restrict__ partials,
            int* __restrict__ out2, unsigned* __restrict__ barrier_state,
            int maxits, double res_atol, double res_rtol, int hier) {
    const long tid = (long)blockIdx.x * BLOCK + threadIdx.x;
    const long nth = (long)gridDim.x * BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice0 = tid >> 6;
    const long nw = nth >> 6;
    bool alive = true;
    auto gsync = [&]() {
        if (alive && !(hier ? grid_barrier_hier(barrier_state)
                            : grid_barrier(barrier_state))) alive = false;
        return alive;
    };

    // grid-wide sum helper: every block contributes partials[bid] (sc1);
    // block 0 reduces into scal[slot]; two grid barriers bracket it.
    auto grid_sum = [&](double v, int slot) {
        v = block_reduce(v);
        if (threadIdx.x == 0) st_sc1_f64(partials + blockIdx.x, v);
        if (!gsync()) return;
        if (blockIdx.x == 0) {
            double s = 0.0;
            for (int i = threadIdx.x; i < (int)gridDim.x; i += BLOCK)
                s += partials[i];
            s = block_reduce(s);
            if (threadIdx.x == 0) st_sc1_f64(scal + slot, s);
        }
        gsync();
    };
    auto spmv = [&](const double* __restrict__ xin, double* __restrict__ yout,
                    bool fuse) -> double {
        double dacc = 0.0;
        for (long s = wslice0; s < nslices; s += nw) {
            const long base = sellptr[s];
            const long len = (sellptr[s + 1] - base) >> 6;
            const double* __restrict__ v = vals + base + lane;
            const ColT* __restrict__ c = cols + base + lane;
            double sum = 0.0;
            long j = 0;
            for (; j + 4 <= len; j += 4) {
                double a0 = ld_nt(v + (j + 0) * WAVE), x0 = xin[c[(j + 0) * WAVE]];
                double a1 = ld_nt(v + (j + 1) * WAVE), x1 = xin[c[(j + 1) * WAVE]];
                double a2 = ld_nt(v + (j + 2) * WAVE), x2 = xin[c[(j + 2) * WAVE]];
                double a3 = ld_nt(v + (j + 3) * WAVE), x3 = xin[c[(j + 3) * WAVE]];
                sum += a0 * x0; sum += a1 * x1; sum += a2 * x2; sum += a3 * x3;
            }
            for (; j < len; ++j) sum += ld_nt(v + j * WAVE) * xin[c[j * WAVE]];
            const long row = s * WAVE + lane;
            if (row < nrows) {
                st_sc1_f64(yout + row, sum);
                if (fuse) dacc += xin[row] * sum;
            }
        }
        return dacc;
    };

    // bnrm2; r0 = b - A x0; p = r0; rr0
    double acc = 0.0;
    for (long i = tid; i < nrows; i += nth) acc += b[i] * b[i];
    grid_sum(acc, S_BNRM2);
    spmv(x, t, false);
    gsync();
    acc = 0.0;
    for (long i = tid; i < nrows; i += nth) {
        const double ri = b[i] - t[i];
        st_sc1_f64(r + i, ri);
        st_sc1_f64(p + i, ri);
        acc += ri * ri;
    }
    grid_sum(acc, S_RR);
    const double bnrm2sqr = alive ? scal[S_BNRM2] : 1.0;
    double rr = alive ? scal[S_RR] : 0.0;
    if (tid == 0) st_sc1_f64(scal + S_RR_PREV, rr);  // report (r0,r0)
    const double rt = res_rtol * sqrt(bnrm2sqr) > res_atol
        ? res_rtol * sqrt(bnrm2sqr) : res_atol;
    const double rtol2 = rt * rt;
    int k = 0, converged = (rtol2 > 0.0 && rr <= rtol2) ? 1 : 0;
    while (alive && !converged && k < maxits) {
        // t = A p (fused (p,t))
        gsync();  // p is consistent (written by all blocks last iter)
        const double pt_part = spmv(p, t, true);
        grid_sum(pt_part, S_PT);
        if (!alive) break;
        const double alpha = safe_div(rr, scal[S_PT]);
        acc = 0.0;
        for (long i = tid; i < nrows; i += nth) {
            const double rn = r[i] - alpha * t[i];
            st_sc1_f64(r + i, rn);
            st_sc1_f64(x + i, x[i] + alpha * p[i]);
            acc += rn * rn;
        }
        grid_sum(acc, S_RR);
        if (!alive) break;
        const double rr_new = scal[S_RR];
        // 0/0-safe like every other CG path: b = 0, or a residual that has
        // underflowed to exact 0, freezes the iterate instead of NaN-ing p
        const double beta = safe_div(rr_new, rr);
        for (long i = tid; i < nrows; i += nth)
            st_sc1_f64(p + i, beta * p[i] + r[i]);
        rr = rr_new;
        ++k;
        if (rtol2 > 0.0 && rr <= rtol2) converged = 1;
    }
    if (tid == 0) {
        st_sc1_f64(scal + S_RR, rr);
        out2[0] = k;
        out2[1] = alive ? converged : -1;
    }
    (void)bnrm2sqr;
}

// fp64 atomic-scatter throughput probe (design study for a
// symmetric-storage SpMV: the transpose half's y updates would be HW
// atomic adds; whether that can beat the full-storage roofline depends
// entirely on sustained global_atomic_add_f64 throughput at realistic
// target distributions).  MODE 0: atomic add; 1: plain store (upper
// bound); 2: gather-read (calibration).
__global__ void __launch_bounds__(BLOCK)
k_atomic_probe(double* __restrict__ y, const int* __restrict__ idx,
               const double* __restrict__ v, long nnz, int mode) {
    const long stride = (long)gridDim.x * BLOCK;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nnz; i += stride) {
        if (mode == 0) unsafeAtomicAdd(&y[idx[i]], v[i]);
        else if (mode == 1) y[idx[i]] = v[i];
        else acc += y[idx[i]] * v[i];
    }
    if (mode == 2 && acc == -1.0) y[0] = acc;  // keep the reads live
}

// halo pack: sendbuf[i] = x[sendidx[i]]
// (reference acghalo_pack_hip_double, halo-kernels-hip.hip:48-103; no unpack
// kernel exists -- ghosts are received in place, see dist/halo.py)
template <typename IdxT>
__global__ void __launch_bounds__(BLOCK)
k_pack_gather(double* __restrict__ sendbuf, const double* __restrict__ x,
              const IdxT* __restrict__ idx, long n) {
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride)
        sendbuf[i] = x[idx[i]];
}

// ---------------------------------------------------------------------------
// Multiple right-hand sides.  A multivector is a contiguous (n, K) fp64
// array, K in {2, 4, 8}: element (i, c) at i*K + c, ghost rows as the
// tail.  The K values of a row are one 16*K/2-byte run, so every gather
// of the operator kernels below is K/2 dwordx4 loads from ONE address
// (K = 8 uses half of a 128 B line instead of 8 B of it), and each matrix
// value / column index is read once for K products.  Scalars: column c
// owns the 8-slot slab at scal + c*S_NSLOTS and the partials range
// [c*MAXG, c*MAXG + gridDim.x).  fp64 operator values only.
typedef double d2_t __attribute__((ext_vector_type(2)));

template <int K>
__device__ __forceinline__ void ld_row(const double* __restrict__ p, double (&v)[K]) {
    const d2_t* __restrict__ q = (const d2_t*)p;
    #pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        const d2_t w = q[h];
        v[2 * h] = w.x;
        v[2 * h + 1] = w.y;
    }
}

template <int K>
__device__ __forceinline__ void st_row(double* __restrict__ p, const double (&v)[K]) {
    d2_t* __restrict__ q = (d2_t*)p;
    #pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        d2_t w;
        w.x = v[2 * h];
        w.y = v[2 * h + 1];
        q[h] = w;
    }
}

// K block sums -> partials[c*MAXG + blockIdx.x]
template <int K>
__device__ __forceinline__ void block_reduce_cols(const double (&d)[K],
                                                  double* __restrict__ partials) {
    #pragma unroll
    for (int c = 0; c < K; ++c) {
        if (c) __syncthreads();  // block_reduce reuses its LDS scratch
        const double v = block_reduce(d[c]);
        if (threadIdx.x == 0) partials[(long)c * MAXG + blockIdx.x] = v;
    }
}

// SELL-C-64 SpMM: Y = A X for K interleaved vectors.  Same arrays as
// k_spmv_sell; lane = row, vals/cols NT (read once).  Unroll depth U: the
// single-vector kernel keeps 8 gathers of 8 B in flight per lane; here a
// gather is K/2 dwordx4 loads, so U = 4 (K = 2) or 2 (K = 4, 8) keeps
// 4..8 16-byte loads in flight while a[U] + xx[U][K] + acc[K] stay well
// inside the register file (no scratch, see profiles/multi_rhs.md).
template <typename ColT, int K, bool FUSE_DOT, bool PERM>
__global__ void __launch_bounds__(BLOCK)
k_spmm_sell(long nslices, long nrows,
            const long* __restrict__ sellptr,
            const ColT* __restrict__ cols,
            const double* __restrict__ vals,
            const double* __restrict__ X,
            double* __restrict__ Y,
            double* __restrict__ partials,
            const int* __restrict__ perm) {
    constexpr int U = (K == 2) ? 4 : 2;
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double dacc[K];
    #pragma unroll
    for (int c = 0; c < K; ++c) dacc[c] = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long base = sellptr[s];
        const long len = (sellptr[s + 1] - base) >> 6;
        const double* __restrict__ v = vals + base + lane;
        const ColT* __restrict__ cp = cols + base + lane;
        double acc[K];
        #pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = 0.0;
        long j = 0;
        for (; j + U <= len; j += U) {
            double a[U], xx[U][K];
            #pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = ld_nt(v + (j + u) * WAVE);
                const long ci = (long)ld_nt(cp + (j + u) * WAVE);
                ld_row<K>(X + ci * K, xx[u]);
            }
            #pragma unroll
            for (int u = 0; u < U; ++u) {
                #pragma unroll
                for (int c = 0; c < K; ++c) acc[c] += a[u] * xx[u][c];
            }
        }
        for (; j < len; ++j) {
            const double a = ld_nt(v + j * WAVE);
            const long ci = (long)ld_nt(cp + j * WAVE);
            double xx[K];
            ld_row<K>(X + ci * K, xx);
            #pragma unroll
            for (int c = 0; c < K; ++c) acc[c] += a * xx[c];
        }
        const long row = PERM ? (long)perm[s * WAVE + lane] : s * WAVE + lane;
        if (row < nrows) {
            st_row<K>(Y + row * K, acc);
            if (FUSE_DOT) {
                double xr[K];
                ld_row<K>(X + row * K, xr);
                #pragma unroll
                for (int c = 0; c < K; ++c) dacc[c] += xr[c] * acc[c];
            }
        }
    }
    if (FUSE_DOT) block_reduce_cols<K>(dacc, partials);
}

// Block-SELL SpMM: the DOF^2 values of a block are loaded once and applied
// to the DOF x K gathered values (one contiguous DOF*K*8-byte run at
// X + cb*DOF*K), acc[DOF][K] in registers.
template <int DOF, int K, bool FUSE_DOT>
__global__ void __launch_bounds__(BLOCK)
k_spmm_bsell(long nslices, long nnodes,
             const long* __restrict__ bptr,
             const int* __restrict__ bcol,
             const double* __restrict__ bvals,
             const double* __restrict__ X,
             double* __restrict__ Y,
             double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long wslice = ((long)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const long nw = ((long)gridDim.x * BLOCK) >> 6;
    double dacc[K];
    #pragma unroll
    for (int c = 0; c < K; ++c) dacc[c] = 0.0;
    for (long s = wslice; s < nslices; s += nw) {
        const long b0 = bptr[s];
        const long blen = (bptr[s + 1] - b0) >> 6;
        const int* __restrict__ cp = bcol + b0 + lane;
        const double* __restrict__ v = bvals + b0 * (DOF * DOF);
        double acc[DOF][K];
        #pragma unroll
        for (int r = 0; r < DOF; ++r) {
            #pragma unroll
            for (int c = 0; c < K; ++c) acc[r][c] = 0.0;
        }
        for (long j = 0; j < blen; ++j) {
            const long cb = (long)ld_nt(cp + j * WAVE);
            const double* __restrict__ xb = X + cb * (DOF * K);
            const double* __restrict__ vj = v + j * (DOF * DOF) * WAVE;
            double a[DOF * DOF];
            #pragma unroll
            for (int k = 0; k < DOF * DOF; ++k)
                a[k] = ld_nt(vj + bval_off<DOF * DOF>(k, lane));
            #pragma unroll
            for (int cc = 0; cc < DOF; ++cc) {
                double xv[K];
                ld_row<K>(xb + cc * K, xv);
                #pragma unroll
                for (int r = 0; r < DOF; ++r) {
                    #pragma unroll
                    for (int c = 0; c < K; ++c) acc[r][c] += a[r * DOF + cc] * xv[c];
                }
            }
        }
        const long node = s * WAVE + lane;
        if (node < nnodes) {
            #pragma unroll
            for (int r = 0; r < DOF; ++r) {
                st_row<K>(Y + (node * DOF + r) * K, acc[r]);
                if (FUSE_DOT) {
                    double xr[K];
                    ld_row<K>(X + (node * DOF + r) * K, xr);
                    #pragma unroll
                    for (int c = 0; c < K; ++c) dacc[c] += xr[c] * acc[r][c];
                }
            }
        }
    }
    if (FUSE_DOT) block_reduce_cols<K>(dacc, partials);
}

// Element-wise multi kernels: FLAT mapping.  A thread owns one 16-byte
// pair (i, c), (i, c+1) per grid stride, so a wave instruction covers one
// contiguous 1 KB run whatever K is.  (One thread per whole row was
// measured first: at K = 8 every dwordx4 instruction then strides 64 B
// across the lanes and the fused update ran at 2.6 TB/s, 604 us against
// 8 x 38 us for the single-vector kernel at 4.1 M rows.)  The grid stride
// is a multiple of K/2 pairs, so a thread keeps the same column pair
// h = threadIdx.x % (K/2) for its whole life and needs two coefficients.
//
// pair_reduce_cols: per-column block sums of the threads' (column 2h,
// column 2h+1) accumulators.  The wave tree stops at offset K/2, which
// leaves lane l < K/2 with the sum over its residue class; the 4 wave
// results meet in LDS and thread c < K publishes column c.
template <int K>
__device__ __forceinline__ void pair_reduce_cols(double a0, double a1,
                                                 double* __restrict__ partials) {
    constexpr int H = K / 2;
    #pragma unroll
    for (int off = WAVE / 2; off >= H; off >>= 1) {
        a0 += __shfl_down(a0, off, WAVE);
        a1 += __shfl_down(a1, off, WAVE);
    }
    __shared__ double w[BLOCK / WAVE][K];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
    if (lane < H) {
        w[wid][2 * lane] = a0;
        w[wid][2 * lane + 1] = a1;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = 0.0;
        #pragma unroll
        for (int q = 0; q < BLOCK / WAVE; ++q) v += w[q][threadIdx.x];
        partials[(long)threadIdx.x * MAXG + blockIdx.x] = v;
    }
}

// per-column dots of two (n, K) multivectors; npairs = n*K/2
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_dot_multi(const double* __restrict__ X, const double* __restrict__ Y,
            long npairs, double* __restrict__ partials) {
    const d2_t* __restrict__ xp = (const d2_t*)X;
    const d2_t* __restrict__ yp = (const d2_t*)Y;
    double a0 = 0.0, a1 = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < npairs; i += stride) {
        const d2_t xv = xp[i], yv = yp[i];
        a0 += xv.x * yv.x;
        a1 += xv.y * yv.y;
    }
    pair_reduce_cols<K>(a0, a1, partials);
}

// grid = K blocks: block c sums column c's partials into slot `slot` of
// column c's slab
__global__ void __launch_bounds__(BLOCK)
k_reduce_partials_multi(const double* __restrict__ partials, int nblocks,
                        double* scal, int slot, int accumulate) {
    const double* __restrict__ pc = partials + (long)blockIdx.x * MAXG;
    double* sc = scal + (long)blockIdx.x * S_NSLOTS;
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) v += pc[i];
    v = block_reduce(v);
    if (threadIdx.x == 0) sc[slot] = accumulate ? sc[slot] + v : v;
}

// classic-CG fused update for K columns: alpha_c = rr_c/pt_c from column
// c's slab; R -= alpha_c T; X += alpha_c P; K partials of the new (r,r).
// Same NT discipline as k_cg_fused_update (T and X single-use streams).
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_cg_fused_update_multi(double* __restrict__ R, double* __restrict__ X,
                        const double* __restrict__ P, const double* __restrict__ T,
                        long npairs, const double* __restrict__ scal,
                        double* __restrict__ partials) {
    const int c0 = 2 * (threadIdx.x % (K / 2));
    const double al0 = safe_div(scal[c0 * S_NSLOTS + S_RR], scal[c0 * S_NSLOTS + S_PT]);
    const double al1 = safe_div(scal[(c0 + 1) * S_NSLOTS + S_RR],
                                scal[(c0 + 1) * S_NSLOTS + S_PT]);
    d2_t* __restrict__ rp = (d2_t*)R;
    d2_t* __restrict__ xp = (d2_t*)X;
    const d2_t* __restrict__ pp = (const d2_t*)P;
    const d2_t* __restrict__ tp = (const d2_t*)T;
    double a0 = 0.0, a1 = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < npairs; i += stride) {
        d2_t rv = rp[i], xv = ld_nt(xp + i);
        const d2_t tv = ld_nt(tp + i), pv = pp[i];
        rv.x = rv.x - al0 * tv.x;
        rv.y = rv.y - al1 * tv.y;
        xv.x = xv.x + al0 * pv.x;
        xv.y = xv.y + al1 * pv.y;
        rp[i] = rv;
        __builtin_nontemporal_store(xv, xp + i);
        a0 += rv.x * rv.x;
        a1 += rv.y * rv.y;
    }
    pair_reduce_cols<K>(a0, a1, partials);
}

// grid = K blocks: block c rotates rr -> rr_prev in column c's slab,
// publishes the new (r,r) there AND in the contiguous rr_out[c] (the host
// convergence test stays one small D2H copy per iteration)
__global__ void __launch_bounds__(BLOCK)
k_cg_finalize_multi(const double* __restrict__ partials, int nblocks,
                    double* scal, double* __restrict__ rr_out) {
    const double* __restrict__ pc = partials + (long)blockIdx.x * MAXG;
    double* sc = scal + (long)blockIdx.x * S_NSLOTS;
    double v = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) v += pc[i];
    v = block_reduce(v);
    if (threadIdx.x == 0) {
        sc[S_RR_PREV] = sc[S_RR];
        sc[S_RR] = v;
        rr_out[blockIdx.x] = v;
    }
}

// P = beta_c P + R with beta_c = scal[c][num]/scal[c][den]
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_daypx_ratio_multi(double* __restrict__ P, const double* __restrict__ R,
                    long npairs, const double* __restrict__ scal, int num, int den) {
    const int c0 = 2 * (threadIdx.x % (K / 2));
    const double b0 = safe_div(scal[c0 * S_NSLOTS + num], scal[c0 * S_NSLOTS + den]);
    const double b1 = safe_div(scal[(c0 + 1) * S_NSLOTS + num],
                               scal[(c0 + 1) * S_NSLOTS + den]);
    d2_t* __restrict__ pp = (d2_t*)P;
    const d2_t* __restrict__ rp = (const d2_t*)R;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < npairs; i += stride) {
        d2_t pv = pp[i];
        const d2_t rv = rp[i];
        pv.x = b0 * pv.x + rv.x;
        pv.y = b1 * pv.y + rv.y;
        pp[i] = pv;
    }
}

// ---------------------------------------------------------------------------
// Block CG (Dubrulle's form with orthonormalised residuals, the QR step as
// Cholesky-QR) for one group of kg <= K columns, K in {2, 4, 8}:
//
//   T = A S (k_spmm_*);  M = S^T T (k_gram_multi);  xi = M^-1, xi C
//   (k_block_coef_alpha);  X += S (xi C), W = Q - T xi, partials of W^T W
//   (k_block_update);  zeta = chol(W^T W)^T, zeta^-1, C <- zeta C, the
//   residual norms (k_block_coef_beta);  Q <- W zeta^-1, S <- Q + S zeta^T
//   (k_block_ortho).
//
// The n-sized kernels map ONE ROW PER THREAD per grid-stride trip: the
// K x K coupling needs the whole row in registers, and a Gram entry is a
// sum over rows.  Grams are reduced like every dot here: K(K+1)/2 block
// partials, summed in a fixed order by the one-block coefficient kernels
// (no floating-point atomics).  The state layout is at the top of the
// file.  Once BS_FLAG is set every kernel of the iteration returns before
// its first store, so X, Q, S, C and rr_out[0..K) keep their values.

static inline long block_grid(long n) {
    long blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > BLOCK_MAXG) blocks = BLOCK_MAXG;
    if (blocks < 1) blocks = 1;
    return blocks;
}

template <int K>
__device__ __forceinline__ void ld_row_nt(const double* __restrict__ p, double (&v)[K]) {
    const d2_t* __restrict__ q = (const d2_t*)p;
    #pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        const d2_t w = ld_nt(q + h);
        v[2 * h] = w.x;
        v[2 * h + 1] = w.y;
    }
}

template <int K>
__device__ __forceinline__ void st_row_nt(double* __restrict__ p, const double (&v)[K]) {
    d2_t* __restrict__ q = (d2_t*)p;
    #pragma unroll
    for (int h = 0; h < K / 2; ++h) {
        d2_t w;
        w.x = v[2 * h];
        w.y = v[2 * h + 1];
        __builtin_nontemporal_store(w, q + h);
    }
}

// acc += upper triangle of x y^T; pair (a, b), a <= b, in row-major order
template <int K>
__device__ __forceinline__ void gram_accum(const double (&x)[K], const double (&y)[K],
                                           double (&acc)[K * (K + 1) / 2]) {
    #pragma unroll
    for (int a = 0; a < K; ++a) {
        #pragma unroll
        for (int b = a; b < K; ++b)
            acc[a * K - (a * (a - 1)) / 2 + (b - a)] += x[a] * y[b];
    }
}

// K(K+1)/2 block sums -> partials[p*BLOCK_MAXG + blockIdx.x]
template <int K>
__device__ __forceinline__ void gram_block_reduce(const double (&acc)[K * (K + 1) / 2],
                                                  double* __restrict__ partials) {
    constexpr int NP = K * (K + 1) / 2;
    __shared__ double w[BLOCK / WAVE][NP];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
    #pragma unroll
    for (int p = 0; p < NP; ++p) {
        double v = acc[p];
        #pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1)
            v += __shfl_down(v, off, WAVE);
        if (lane == 0) w[wid][p] = v;
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        double v = 0.0;
        #pragma unroll
        for (int q = 0; q < BLOCK / WAVE; ++q) v += w[q][threadIdx.x];
        partials[(long)threadIdx.x * BLOCK_MAXG + blockIdx.x] = v;
    }
}

// upper triangle of X^T Y over the first n rows
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_gram_multi(const double* __restrict__ X, const double* __restrict__ Y,
             long n, double* __restrict__ partials) {
    double acc[K * (K + 1) / 2];
    #pragma unroll
    for (int p = 0; p < K * (K + 1) / 2; ++p) acc[p] = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        double x[K], y[K];
        ld_row<K>(X + i * K, x);
        ld_row<K>(Y + i * K, y);
        gram_accum<K>(x, y, acc);
    }
    gram_block_reduce<K>(acc, partials);
}

// X += S (xi C);  W = Q - T xi over Q;  block partials of W^T W.  The
// 2 K^2 coefficients are staged in LDS once per block (broadcast reads).
// X and T are single-use streams (NT), S and Q are read again by
// k_block_ortho.
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_block_update(double* __restrict__ X, const double* __restrict__ S,
               double* __restrict__ Q, const double* __restrict__ T, long n,
               const double* __restrict__ state, double* __restrict__ partials) {
    if (state[BS_FLAG] != 0.0) return;
    __shared__ double cxi[K * K], cxc[K * K];
    if (threadIdx.x < K * K) {
        const int a = threadIdx.x / K, c = threadIdx.x % K;
        cxi[threadIdx.x] = state[BS_XI + a * BS_LD + c];
        cxc[threadIdx.x] = state[BS_XIC + a * BS_LD + c];
    }
    __syncthreads();
    double acc[K * (K + 1) / 2];
    #pragma unroll
    for (int p = 0; p < K * (K + 1) / 2; ++p) acc[p] = 0.0;
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        // keep the LDS coefficient reads inside the trip: hoisted out of
        // the loop, the 2 K^2 values alone fill the register file at K = 8
        asm volatile("" ::: "memory");
        double s[K], x[K], t[K], w[K];
        ld_row<K>(S + i * K, s);
        ld_row_nt<K>(X + i * K, x);
        ld_row_nt<K>(T + i * K, t);
        ld_row<K>(Q + i * K, w);
        #pragma unroll
        for (int a = 0; a < K; ++a) {
            #pragma unroll
            for (int c = 0; c < K; ++c) x[c] += s[a] * cxc[a * K + c];
        }
        st_row_nt<K>(X + i * K, x);
        #pragma unroll
        for (int a = 0; a < K; ++a) {
            #pragma unroll
            for (int c = 0; c < K; ++c) w[c] -= t[a] * cxi[a * K + c];
        }
        st_row<K>(Q + i * K, w);
        gram_accum<K>(w, w, acc);
    }
    gram_block_reduce<K>(acc, partials);
}

// Q <- W zeta^-1;  S <- Q + S zeta^T on the first n rows.  (NT accesses
// for Q, meant to keep S cache-resident for the SpMM that follows, were
// measured and bought nothing: profiles/block_cg.md.)
template <int K>
__global__ void __launch_bounds__(BLOCK)
k_block_ortho(double* __restrict__ Q, double* __restrict__ S, long n,
              const double* __restrict__ state) {
    if (state[BS_FLAG] != 0.0) return;
    __shared__ double czi[K * K], cz[K * K];
    if (threadIdx.x < K * K) {
        const int a = threadIdx.x / K, c = threadIdx.x % K;
        czi[threadIdx.x] = state[BS_ZINV + a * BS_LD + c];
        cz[threadIdx.x] = state[BS_ZETA + a * BS_LD + c];
    }
    __syncthreads();
    const long stride = (long)gridDim.x * BLOCK;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        asm volatile("" ::: "memory");  // as in k_block_update
        double w[K], s[K], q[K], sn[K];
        ld_row<K>(Q + i * K, w);
        ld_row<K>(S + i * K, s);
        #pragma unroll
        for (int c = 0; c < K; ++c) q[c] = 0.0;
        #pragma unroll
        for (int a = 0; a < K; ++a) {
            #pragma unroll
            for (int c = 0; c < K; ++c) q[c] += w[a] * czi[a * K + c];
        }
        #pragma unroll
        for (int c = 0; c < K; ++c) sn[c] = q[c];
        #pragma unroll
        for (int a = 0; a < K; ++a) {
            #pragma unroll
            for (int c = 0; c < K; ++c) sn[c] += s[a] * cz[c * K + a];  // zeta^T
        }
        st_row<K>(Q + i * K, q);
        st_row<K>(S + i * K, sn);
    }
}

// One workgroup: sum the Gram partials of every pair into the upper
// triangle of g.  64 / 16 / 4 threads per pair (K = 2 / 4 / 8: the largest
// power of two with pairs * threads <= BLOCK), each summing a fixed strided
// subsequence in four independent accumulators (the loads pipeline instead
// of waiting on one add chain), joined by xor shuffles (a + b on both
// sides, so every thread of a pair holds the same bits).
__device__ __forceinline__ void block_sum_pairs(const double* __restrict__ partials,
                                                int nblocks, int K,
                                                double (*g)[BS_LD]) {
    const int tpp = K == 2 ? 64 : (K == 4 ? 16 : 4);
    const int p = threadIdx.x / tpp, sub = threadIdx.x % tpp;
    const int np = K * (K + 1) / 2;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (p < np) {
        const double* __restrict__ q = partials + (long)p * BLOCK_MAXG;
        int i = sub;
        for (; i + 3 * tpp < nblocks; i += 4 * tpp) {
            a0 += q[i];
            a1 += q[i + tpp];
            a2 += q[i + 2 * tpp];
            a3 += q[i + 3 * tpp];
        }
        for (; i < nblocks; i += tpp) a0 += q[i];
    }
    double v = (a0 + a1) + (a2 + a3);
    for (int off = 1; off < tpp; off <<= 1) v += __shfl_xor(v, off, WAVE);
    if (sub == 0 && p < np) {
        int a = 0, q = p;
        while (q >= K - a) { q -= K - a; ++a; }
        g[a][a + q] = v;
    }
}

// Pivot-tested Cholesky g = l l^T of the leading kg x kg block (serial,
// one thread; l starts as the identity).  Pivot d_j is tested against the
// diagonal entry it came from: d_j / g_jj is the squared sine of the angle
// between column j and the span of the columns before it.
__device__ __forceinline__ bool block_chol(const double (*g)[BS_LD],
                                           double (*l)[BS_LD], int kg) {
    for (int j = 0; j < kg; ++j) {
        double d = g[j][j];
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        if (!__builtin_isfinite(d) || !(d > BLOCK_TAU * g[j][j])) return false;
        const double ljj = sqrt(d);
        l[j][j] = ljj;
        for (int i = j + 1; i < kg; ++i) {
            double s = g[i][j];
            for (int k = 0; k < j; ++k) s -= l[i][k] * l[j][k];
            l[i][j] = s / ljj;
        }
    }
    return true;
}

// sums -> symmetric g with rows/cols >= kg the identity; l = identity.
// Returns this thread's entry of g (threads < 64: a = t/8, b = t%8).
__device__ __forceinline__ double block_gram_setup(const double* __restrict__ partials,
                                                   int nblocks, int K, int kg,
                                                   double (*g)[BS_LD],
                                                   double (*l)[BS_LD]) {
    const int a = threadIdx.x >> 3, b = threadIdx.x & 7;
    block_sum_pairs(partials, nblocks, K, g);
    if (threadIdx.x < 64) l[a][b] = (a == b) ? 1.0 : 0.0;
    __syncthreads();
    double m = 0.0;
    if (threadIdx.x < 64)
        m = (a < kg && b < kg) ? (a <= b ? g[a][b] : g[b][a]) : (a == b ? 1.0 : 0.0);
    __syncthreads();
    if (threadIdx.x < 64) g[a][b] = m;
    __syncthreads();
    return m;
}

// M from the partials, xi = M^-1 (column c: L y = e_c, L^T x = y, so the
// backward error of a Cholesky solve holds per column), xi C
__global__ void __launch_bounds__(BLOCK)
k_block_coef_alpha(const double* __restrict__ partials, int nblocks,
                   double* state, int K, int kg, int it) {
    if (state[BS_FLAG] != 0.0) return;
    __shared__ double g[BS_LD][BS_LD], l[BS_LD][BS_LD], xi[BS_LD][BS_LD];
    __shared__ int ok;
    const int t = threadIdx.x, a = t >> 3, b = t & 7;
    const bool mine = t < 64 && a < K && b < K;
    const double m = block_gram_setup(partials, nblocks, K, kg, g, l);
    if (t < 64) xi[a][b] = (a == b) ? 1.0 : 0.0;
    if (t == 0) ok = block_chol(g, l, kg) ? 1 : 0;
    __syncthreads();
    if (mine) state[BS_M + a * BS_LD + b] = m;
    if (!ok) {
        if (t == 0) {
            state[BS_FLAG] = 1.0;
            state[BS_ITER] = (double)it;
        }
        return;
    }
    if (t < kg) {
        const int c = t;
        for (int i = c; i < kg; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= l[i][k] * xi[k][c];
            xi[i][c] = s / l[i][i];
        }
        for (int i = kg - 1; i >= 0; --i) {
            double s = xi[i][c];
            for (int k = i + 1; k < kg; ++k) s -= l[k][i] * xi[k][c];
            xi[i][c] = s / l[i][i];
        }
    }
    __syncthreads();
    if (mine) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += xi[a][k] * state[BS_C + k * BS_LD + b];
        state[BS_XI + a * BS_LD + b] = xi[a][b];
        state[BS_XIC + a * BS_LD + b] = s;
    }
}

// G from the partials, zeta = chol(G)^T, zeta^-1 (column c by back
// substitution of zeta x = e_c), C <- zeta C (init: C = zeta),
// rr_out[c] = ||C[:, c]||^2 for c < kg, rr_out[K] / rr_out[K+1] = flag /
// iteration.  With the flag already set only the latter two are written,
// so a breakdown found by k_block_coef_alpha reaches the host copy too.
__global__ void __launch_bounds__(BLOCK)
k_block_coef_beta(const double* __restrict__ partials, int nblocks,
                  double* state, double* __restrict__ rr_out, int K, int kg,
                  int it, int init) {
    const int t = threadIdx.x, a = t >> 3, b = t & 7;
    if (state[BS_FLAG] != 0.0) {
        if (t == 0) {
            rr_out[K] = state[BS_FLAG];
            rr_out[K + 1] = state[BS_ITER];
        }
        return;
    }
    __shared__ double g[BS_LD][BS_LD], l[BS_LD][BS_LD], zi[BS_LD][BS_LD],
                      cs[BS_LD][BS_LD];
    __shared__ int ok;
    const bool mine = t < 64 && a < K && b < K;
    const double m = block_gram_setup(partials, nblocks, K, kg, g, l);
    if (t < 64) zi[a][b] = (a == b) ? 1.0 : 0.0;
    if (t == 0) ok = block_chol(g, l, kg) ? 1 : 0;
    __syncthreads();
    if (mine) state[BS_G + a * BS_LD + b] = m;
    if (!ok) {
        if (t == 0) {
            state[BS_FLAG] = 1.0;
            state[BS_ITER] = (double)it;
            rr_out[K] = 1.0;
            rr_out[K + 1] = (double)it;
        }
        return;
    }
    if (t < kg) {
        const int c = t;
        for (int i = c; i >= 0; --i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = i + 1; k <= c; ++k) s -= l[k][i] * zi[k][c];
            zi[i][c] = s / l[i][i];
        }
    }
    double cn = 0.0;
    if (mine) {
        if (init) {
            cn = l[b][a];
        } else {
            for (int k = 0; k < K; ++k) cn += l[k][a] * state[BS_C + k * BS_LD + b];
        }
        cs[a][b] = cn;
    }
    __syncthreads();  // every read of the old C is done; zi and cs complete
    if (mine) {
        state[BS_ZETA + a * BS_LD + b] = l[b][a];
        state[BS_ZINV + a * BS_LD + b] = zi[a][b];
        state[BS_C + a * BS_LD + b] = cn;
    }
    if (t < kg) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += cs[k][t] * cs[k][t];
        rr_out[t] = s;
    }
    if (t == 0) {
        rr_out[K] = 0.0;
        rr_out[K + 1] = -1.0;
    }
}

// ---------------------------------------------------------------------------
// host-side launchers (pybind).  Tensors arrive as raw device pointers +
// sizes + the caller's HIP stream handle (torch.cuda.current_stream().cuda_stream);
// no torch C++ dependency, no hipify, plain HIP throughout.
//
// A launcher validates, sizes the grid, then turns its runtime selectors
// into template arguments with the dispatch helpers below and launches
// through launch().  Every instantiation that exists is spelled as a
// kernel<...> expression inside a launcher; nothing else instantiates one.

using std::uintptr_t;

static inline hipStream_t S(uintptr_t s) { return (hipStream_t)s; }

// -- dispatch helpers: runtime selector -> compile-time argument ------------
// Each calls the generic lambda ``f`` with a tag object whose type carries
// the value.  A tag parameter converts to its value in a constant
// expression (``k<d, fd>``); a lambda nested inside needs it re-declared
// as a constexpr local first (``constexpr int D = d;``), since a captured
// parameter is no constant.

template <typename T> struct type_tag { using type = T; };

template <typename F>
static inline void dispatch_bool(bool v, F&& f) {
    if (v) f(std::true_type{}); else f(std::false_type{});
}

template <typename F>
static inline void dispatch_bool(bool v0, bool v1, F&& f) {
    dispatch_bool(v0, [&](auto b0) {
        dispatch_bool(v1, [&](auto b1) { f(b0, b1); });
    });
}

// ``v`` must be one of Vs..., else Err(who + rule) is thrown
template <typename Err, int... Vs, typename F>
static inline void dispatch_int(int v, const char* who, const char* rule, F&& f) {
    const bool hit =
        ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    if (!hit) throw Err(std::string(who) + rule);
}

template <typename F>
static inline void dispatch_dof(int dof, const char* who, F&& f) {
    dispatch_int<std::runtime_error, 2, 3, 4>(dof, who, ": dof must be 2/3/4", f);
}

template <typename F>
static inline void dispatch_k(int k, const char* who, F&& f) {
    dispatch_int<std::invalid_argument, 2, 4, 8>(k, who, ": K must be 2, 4 or 8", f);
}

// f(type_tag<T1>) if v else f(type_tag<T0>)
template <typename T1, typename T0, typename F>
static inline void dispatch_type(bool v, F&& f) {
    if (v) f(type_tag<T1>{}); else f(type_tag<T0>{});
}

// col64 / idx64 flag -> long / int indices
template <typename F>
static inline void dispatch_index(int is64, F&& f) {
    dispatch_type<long, int>(is64 != 0, f);
}

// val32 flag -> fp32- / fp64-stored operator values
template <typename F>
static inline void dispatch_value(bool val32, F&& f) {
    dispatch_type<float, double>(val32, f);
}

// -- grids --------------------------------------------------------------------

// one wave per 64-row slice, BLOCK/WAVE slices per block; grid-stride
// takes what MAXG cuts off
static inline long slice_grid(long nslices) {
    long blocks = (nslices * WAVE + BLOCK - 1) / BLOCK;
    if (blocks > MAXG) blocks = MAXG;
    return blocks;
}

// Megafused passes write their partials at partials_off + blockIdx.x.  The
// matA pass (partials_off == 0) must leave partial slots for the matO
// pass: at >=3.9M rows an uncapped matA claims all MAXG blocks and matO
// would launch with grid 0 (invalid configuration), so 1024 are reserved.
static inline long pipe_grid(long blocks, long partials_off) {
    const long cap = (partials_off == 0) ? (MAXG - 1024) : (MAXG - partials_off);
    if (blocks > cap) blocks = cap;
    return blocks;
}

// block-Jacobi: one thread per node, ~2 nodes per thread before the cap
static inline long bj_grid(long nnodes) { return elem_grid(nnodes, 2); }

// -- launch -------------------------------------------------------------------
// Arguments are checked against the kernel's parameter list: a pointer
// parameter takes a uintptr_t (the only conversion made) or a pointer of
// exactly its type, any other parameter an argument of exactly its type.
// An int for a pointer, or a long for an int, does not compile.

template <typename P, typename A>
static inline P kernel_arg(A a) {
    if constexpr (std::is_pointer_v<P> && std::is_same_v<A, uintptr_t>) {
        return reinterpret_cast<P>(a);
    } else {
        static_assert(std::is_same_v<P, A>,
                      "kernel argument: uintptr_t for a pointer, else the exact type");
        return a;
    }
}

template <typename... P, typename... A>
static inline void launch_cfg(const char* what, void (*kern)(P...), dim3 grid,
                              dim3 block, size_t lds, uintptr_t stream, A... args) {
    static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
    hipLaunchKernelGGL(kern, grid, block, lds, S(stream), kernel_arg<P>(args)...);
    check_hip(what);
}

// the common shape: ``blocks`` x BLOCK threads, no dynamic LDS
template <typename... P, typename... A>
static inline void launch(const char* what, void (*kern)(P...), long blocks,
                          uintptr_t stream, A... args) {
    launch_cfg(what, kern, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, args...);
}

static void reduce_partials(uintptr_t partials, int nblocks, uintptr_t scal,
                            int slot, bool accumulate, uintptr_t stream) {
    launch("reduce_partials", k_reduce_partials, 1, stream, partials, nblocks,
           scal, slot, accumulate ? 1 : 0);
}

// -- CSR / SELL SpMV ----------------------------------------------------------

void spmv(long nrows, long rowbase, uintptr_t rowptr, uintptr_t colidx,
          int col64, uintptr_t vals, uintptr_t x, uintptr_t y,
          int lanes, bool accum, uintptr_t partials, uintptr_t scal,
          int dotslot, bool dot_accum, uintptr_t stream) {
    if (nrows == 0) return;
    const int rows_per_block = BLOCK / lanes;
    long blocks = (nrows + rows_per_block - 1) / rows_per_block;
    if (blocks > MAXG) blocks = MAXG;
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_index(col64, [&](auto ct) {
        using CT = typename decltype(ct)::type;
        dispatch_int<std::runtime_error, 4, 8, 16, 32, 64>(
            lanes, "spmv", ": lanes must be 4/8/16/32/64", [&](auto l) {
                constexpr int L = l;
                dispatch_bool(accum, fuse, [&](auto ac, auto fd) {
                    launch("spmv", spmv_csr_vector<CT, L, ac, fd>, blocks, stream,
                           nrows, rowbase, rowptr, colidx, vals, x, y, partials,
                           uintptr_t(0));
                });
            });
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
}

// Row-binned hybrid CSR SpMV: rows pre-sorted by length into bins, one
// launch per bin with bin-appropriate LANES (4..64).  Every row is fully
// reduced by one lane group => deterministic, no atomics; each launch
// writes its own partials window, one finalize over the union.  This is
// the MI355X-native load-balancer for power-law rows (reference analog:
// merge-path csrgemv_merge, cg-kernels-hip.hip:348-1175).
// bins: (start_in_rowlist, count, lanes) triples.
void spmv_binned(long rowbase, uintptr_t rowptr, uintptr_t colidx, int col64,
                 uintptr_t vals, uintptr_t x, uintptr_t y, uintptr_t rowlist,
                 const std::vector<std::array<long, 3>>& bins,
                 bool accum, uintptr_t partials, uintptr_t scal,
                 int dotslot, bool dot_accum, uintptr_t stream) {
    const bool fuse = partials != 0 && dotslot >= 0;
    long poff = 0;
    for (const auto& bin : bins) {
        const long start = bin[0], count = bin[1];
        const int lanes = (int)bin[2];
        if (count == 0) continue;
        const int rows_per_block = BLOCK / lanes;
        long blocks = (count + rows_per_block - 1) / rows_per_block;
        if (blocks > 3072) blocks = 3072;  // grid-stride within the bin
        // (5 bins x 3072 <= MAXG partials)
        if (poff + blocks > MAXG)
            throw std::runtime_error("spmv_binned: partials overflow");
        const int* rl = (const int*)rowlist + start;
        double* pp = (double*)partials + poff;
        dispatch_index(col64, [&](auto ct) {
            using CT = typename decltype(ct)::type;
            dispatch_int<std::runtime_error, 4, 8, 16, 32, 64>(
                lanes, "spmv_binned", ": lanes 4/8/16/32/64", [&](auto l) {
                    constexpr int L = l;
                    dispatch_bool(accum, fuse, [&](auto ac, auto fd) {
                        launch("spmv_binned", spmv_csr_vector<CT, L, ac, fd, true>,
                               blocks, stream, count, rowbase, rowptr, colidx,
                               vals, x, y, pp, rl);
                    });
                });
        });
        if (fuse) poff += blocks;
    }
    if (fuse && poff > 0)
        reduce_partials(partials, (int)poff, scal, dotslot, dot_accum, stream);
}

void spmv_sell(long nslices, long nrows, long rowbase, uintptr_t sellptr,
               uintptr_t cols, int col64, uintptr_t vals, uintptr_t x,
               uintptr_t y, bool accum, uintptr_t partials, uintptr_t scal,
               int dotslot, bool dot_accum, int variant, uintptr_t perm,
               bool val32, uintptr_t stream) {
    if (nrows == 0) return;
    const long blocks = slice_grid(nslices);
    const bool fuse = partials != 0 && dotslot >= 0;
    const int flavour = variant & (SELL_NT | SELL_SWZ | SELL_U8);
    if (val32 && flavour != (SELL_NT | SELL_U8))
        throw std::invalid_argument(
            "spmv_sell: fp32 values support only variant NT|U8");
    dispatch_index(col64, [&](auto ct) {
        using CT = typename decltype(ct)::type;
        dispatch_bool(accum, fuse, [&](auto ac, auto fd) {
            constexpr bool AC = ac, FD = fd;
            auto go = [&](auto kern) {
                launch("spmv_sell", kern, blocks, stream, nslices, nrows, rowbase,
                       sellptr, cols, vals, x, y, partials, perm);
            };
            if (val32) {
                // fp32-stored values: only the default flavour (NT, no SWZ,
                // unroll 8), plain or sigma-perm, is instantiated
                dispatch_bool(perm != 0, [&](auto pm) {
                    go(k_spmv_sell<CT, AC, FD, true, false, 8, pm, float>);
                });
            } else if (perm != 0) {
                // sigma-sorted SELL (irregular rows): fixed NT, no swizzle;
                // UNROLL honours the U8 variant bit (deeper unroll = more
                // outstanding x gathers to hide the random-access latency
                // that dominates this path)
                dispatch_bool((variant & SELL_U8) != 0, [&](auto u8) {
                    go(k_spmv_sell<CT, AC, FD, true, false, u8 ? 8 : 4, true>);
                });
            } else {
                dispatch_int<std::logic_error, 0, 1, 2, 3, 4, 5, 6, 7>(
                    flavour, "spmv_sell", ": variant", [&](auto v) {
                        constexpr int V = v;
                        go(k_spmv_sell<CT, AC, FD, (V & SELL_NT) != 0,
                                       (V & SELL_SWZ) != 0, (V & SELL_U8) ? 8 : 4>);
                    });
            }
        });
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
}

// Dual SpMV launchers (residual replacement).  ``b`` != 0 selects RESID,
// ``partials`` != 0 the fused (x1,x1) / (y1,x1) partials; both return the
// number of blocks launched (= partials written per half when fused).
long spmv2_sell(long nslices, long nrows, uintptr_t sellptr, uintptr_t cols,
                int col64, uintptr_t vals, uintptr_t x1, uintptr_t x2,
                uintptr_t b, uintptr_t y1, uintptr_t y2, uintptr_t partials,
                uintptr_t perm, uintptr_t stream) {
    if (nrows == 0 || nslices == 0) return 0;
    const long blocks = slice_grid(nslices);
    dispatch_index(col64, [&](auto ct) {
        using CT = typename decltype(ct)::type;
        dispatch_bool(b != 0, partials != 0, [&](auto rs, auto fd) {
            constexpr bool RS = rs, FD = fd;
            dispatch_bool(perm != 0, [&](auto pm) {
                launch("spmv2_sell", k_spmv2_sell<CT, RS, FD, pm>, blocks, stream,
                       nslices, nrows, sellptr, cols, vals, x1, x2, b, y1, y2,
                       partials, perm);
            });
        });
    });
    return blocks;
}

// dof 1 = SELL rows (optional sigma perm), dof 2/3/4 = BSELL nodes
long dot2_slices(long nslices, long nunits, int dof, uintptr_t r, uintptr_t w,
                 uintptr_t perm, uintptr_t partials, uintptr_t stream) {
    if (dof < 1 || dof > 4 || (dof > 1 && perm != 0))
        throw std::runtime_error("dot2_slices: dof must be 1..4, perm only with dof 1");
    if (nunits == 0 || nslices == 0) return 0;
    const long blocks = slice_grid(nslices);
    auto go = [&](auto kern) {
        launch("dot2_slices", kern, blocks, stream, nslices, nunits, r, w, perm,
               partials);
    };
    dispatch_int<std::runtime_error, 1, 2, 3, 4>(
        dof, "dot2_slices", ": dof must be 1..4", [&](auto d) {
            if constexpr (d == 1)
                dispatch_bool(perm != 0, [&](auto pm) { go(k_dot2_slices<1, pm>); });
            else
                go(k_dot2_slices<d, false>);
        });
    return blocks;
}

// -- Block-SELL ---------------------------------------------------------------

void spmv_bsell(long nslices, long nnodes, int dof, uintptr_t bptr,
                uintptr_t bcol, uintptr_t bvals, uintptr_t x, uintptr_t y,
                uintptr_t partials, uintptr_t scal, int dotslot,
                bool dot_accum, bool val32, uintptr_t stream) {
    if (nnodes == 0) return;
    const long blocks = slice_grid(nslices);
    const bool fuse = partials != 0 && dotslot >= 0;
    // fp32-stored values keep the same pair-major element order
    dispatch_value(val32, [&](auto vt) {
        using VT = typename decltype(vt)::type;
        dispatch_dof(dof, "spmv_bsell", [&](auto d) {
            constexpr int D = d;
            dispatch_bool(fuse, [&](auto fd) {
                launch("spmv_bsell", k_spmv_bsell<D, fd, VT>, blocks, stream,
                       nslices, nnodes, bptr, bcol, bvals, x, y, partials);
            });
        });
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
}

// Returns the number of blocks launched (= partials written when fused).
// ``max_blocks`` > 0 caps the grid (grid-stride over tiles takes the rest).
long spmv_bsell_st(long ntiles, long nslices, long nnodes, int dof, int qmax,
                   uintptr_t sptr, uintptr_t spl, uintptr_t scol, uintptr_t sq,
                   uintptr_t svals, uintptr_t nrecv, uintptr_t x, uintptr_t y,
                   uintptr_t partials, uintptr_t scal, int dotslot,
                   bool dot_accum, long max_blocks, uintptr_t stream) {
    if (nnodes == 0 || ntiles == 0) return 0;
    if (ntiles != (nslices + BLOCK / WAVE - 1) / (BLOCK / WAVE)
        || nslices != (nnodes + WAVE - 1) / WAVE)
        throw std::invalid_argument("spmv_bsell_st: tile/slice/node counts disagree");
    if (qmax < 0 || qmax >= ST_NOSEND)
        throw std::invalid_argument("spmv_bsell_st: qmax must be in [0, 255)");
    const size_t lds = (size_t)qmax * dof * BLOCK * sizeof(double);
    if (lds > 96 * 1024)
        throw std::invalid_argument("spmv_bsell_st: qmax * dof needs more than 96 KiB of LDS");
    long blocks = ntiles;
    if (blocks > MAXG) blocks = MAXG;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_dof(dof, "spmv_bsell_st", [&](auto d) {
        constexpr int D = d;
        dispatch_bool(fuse, [&](auto fd) {
            auto kern = k_spmv_bsell_st<D, fd>;
            if (lds > 48 * 1024 && hipFuncSetAttribute(
                    (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                    (int)lds) != hipSuccess)
                throw std::runtime_error("spmv_bsell_st: cannot raise the LDS limit");
            launch_cfg("spmv_bsell_st", kern, dim3((unsigned)blocks), dim3(BLOCK),
                       lds, stream, ntiles, nslices, nnodes, sptr, spl, scol, sq,
                       svals, nrecv, x, y, partials);
        });
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
    return blocks;
}

void spmv_bsell_daypx(long nslices, long nnodes, int dof, uintptr_t bptr,
                      uintptr_t bcol, uintptr_t bvals, uintptr_t pold,
                      uintptr_t rvec, uintptr_t pnew, uintptr_t y,
                      uintptr_t scal, uintptr_t partials, int dotslot,
                      uintptr_t stream) {
    if (nnodes == 0) return;
    const long blocks = slice_grid(nslices);
    dispatch_dof(dof, "spmv_bsell_daypx", [&](auto d) {
        launch("spmv_bsell_daypx", k_spmv_bsell_daypx<d>, blocks, stream, nslices,
               nnodes, bptr, bcol, bvals, pold, rvec, pnew, y, scal, partials);
    });
    reduce_partials(partials, (int)blocks, scal, dotslot, false, stream);
}

long spmv2_bsell(long nslices, long nnodes, int dof, uintptr_t bptr,
                 uintptr_t bcol, uintptr_t bvals, uintptr_t x1, uintptr_t x2,
                 uintptr_t b, uintptr_t y1, uintptr_t y2, uintptr_t partials,
                 uintptr_t stream) {
    if (dof < 2 || dof > 4)
        throw std::runtime_error("spmv2_bsell: dof must be 2/3/4");
    if (nnodes == 0 || nslices == 0) return 0;
    const long blocks = slice_grid(nslices);
    dispatch_dof(dof, "spmv2_bsell", [&](auto d) {
        constexpr int D = d;
        dispatch_bool(b != 0, partials != 0, [&](auto rs, auto fd) {
            launch("spmv2_bsell", k_spmv2_bsell<D, rs, fd>, blocks, stream, nslices,
                   nnodes, bptr, bcol, bvals, x1, x2, b, y1, y2, partials);
        });
    });
    return blocks;
}

void bsell_diag_inv(long nslices, long nnodes, int dof, uintptr_t bptr,
                    uintptr_t bcol, uintptr_t bvals, uintptr_t minv,
                    uintptr_t status, uintptr_t stream) {
    if (nnodes == 0) return;
    const long blocks = slice_grid(nslices);
    dispatch_dof(dof, "bsell_diag_inv", [&](auto d) {
        launch("bsell_diag_inv", k_bsell_diag_inv<d>, blocks, stream, nslices,
               nnodes, bptr, bcol, bvals, minv, status);
    });
}

void bjacobi_apply(uintptr_t minv, uintptr_t r, uintptr_t z, long nnodes,
                   int dof, uintptr_t scal, uintptr_t partials,
                   uintptr_t stream) {
    const long blocks = bj_grid(nnodes);
    dispatch_dof(dof, "bjacobi_apply", [&](auto d) {
        launch("bjacobi_apply", k_bjacobi_apply<d>, blocks, stream, minv, r, z,
               nnodes, partials);
    });
    launch("bjacobi_apply", k_pcg_finalize, 1, stream, partials, (int)blocks, scal);
}

void bpcg_fused_update(uintptr_t r, uintptr_t x, uintptr_t p, uintptr_t t,
                       uintptr_t z, uintptr_t minv, long nnodes, int dof,
                       uintptr_t scal, uintptr_t partials, uintptr_t stream) {
    const long blocks = bj_grid(nnodes);
    dispatch_dof(dof, "bpcg_fused_update", [&](auto d) {
        launch("bpcg_fused_update", k_bpcg_fused_update<d>, blocks, stream, r, x,
               p, t, z, minv, nnodes, scal, partials);
    });
    launch("bpcg_fused_update", k_pcg_finalize, 1, stream, partials, (int)blocks,
           scal);
}

// -- slab generators ----------------------------------------------------------

void stencil_blocklen(long nnodes, int gx, int gy, int gz, long nown_nodes,
                      uintptr_t zs_of_plane, uintptr_t pb, uintptr_t offs,
                      int ksten, uintptr_t blocklen, uintptr_t stream) {
    launch("stencil_blocklen", k_stencil_blocklen, elem_grid(nnodes), stream,
           nnodes, gx, gy, gz, nown_nodes, zs_of_plane, pb, offs, ksten, blocklen);
}

void stencil_bfill(long nnodes, int gx, int gy, int gz, int dof,
                   long nown_nodes, uintptr_t zs_of_plane, uintptr_t pb,
                   uintptr_t offs, int ksten, uintptr_t blocks_md,
                   uintptr_t bptr, uintptr_t bcol, uintptr_t bvals,
                   uintptr_t stream) {
    dispatch_dof(dof, "stencil_bfill", [&](auto d) {
        launch("stencil_bfill", k_stencil_bfill<d>, elem_grid(nnodes), stream,
               nnodes, gx, gy, gz, nown_nodes, zs_of_plane, pb, offs, ksten,
               blocks_md, bptr, bcol, bvals);
    });
}

void stencil_rowlen(long nrows_nodes, long row0_node, int gx, int gy, int gz,
                    int dof, long nown_nodes, uintptr_t zs_of_plane,
                    uintptr_t pb, uintptr_t offs, int ksten, int filter_ghost,
                    uintptr_t rowlen, uintptr_t stream) {
    launch("stencil_rowlen", k_stencil_rowlen, elem_grid(nrows_nodes), stream,
           nrows_nodes, row0_node, gx, gy, gz, dof, nown_nodes, zs_of_plane, pb,
           offs, ksten, filter_ghost, rowlen);
}

void stencil_fill(long nrows_nodes, long row0_node, int gx, int gy, int gz,
                  int dof, long nown_nodes, uintptr_t zs_of_plane,
                  uintptr_t pb, uintptr_t offs, int ksten, uintptr_t blocks,
                  int filter_ghost, uintptr_t sellptr, uintptr_t cols,
                  uintptr_t vals, uintptr_t stream) {
    const long nrows = nrows_nodes * dof;
    launch("stencil_fill", k_stencil_fill, elem_grid(nrows), stream, nrows_nodes,
           row0_node, gx, gy, gz, dof, nown_nodes, zs_of_plane, pb, offs, ksten,
           blocks, filter_ghost, sellptr, cols, vals);
}

// -- matrix-free stencils -----------------------------------------------------

void stencil_spmv7(long plane_nodes, int gx, int z0, int z1, int gz,
                   long nown_nodes, uintptr_t pb, double diag,
                   double wxm, double wxp, double wym, double wyp,
                   double wzm, double wzp, uintptr_t x, uintptr_t y,
                   uintptr_t partials, uintptr_t scal, int dotslot,
                   bool dot_accum, uintptr_t stream) {
    if (plane_nodes == 0 || z1 <= z0) return;
    long blocks = (plane_nodes + BLOCK - 1) / BLOCK;
    if (blocks > MAXG) blocks = MAXG;
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_bool(fuse, [&](auto fd) {
        launch("stencil_spmv7", k_stencil_spmv7<fd>, blocks, stream, plane_nodes,
               gx, z0, z1, gz, nown_nodes, pb, diag, wxm, wxp, wym, wyp, wzm, wzp,
               x, y, partials);
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
}

long stencil_pipe7(long plane_nodes, int gx, int z0, int z1, int gz,
                   long border_base, long nown_nodes, uintptr_t pb,
                   double diag, double wxm, double wxp, double wym,
                   double wyp, double wzm, double wzp, uintptr_t w_old,
                   uintptr_t qpart, uintptr_t z, uintptr_t t, uintptr_t p,
                   uintptr_t xv, uintptr_t r, uintptr_t w_new, uintptr_t scal,
                   int first, uintptr_t partials, long partials_off,
                   uintptr_t stream) {
    if (plane_nodes == 0 || z1 <= z0) return 0;
    const long blocks = pipe_grid((plane_nodes + BLOCK - 1) / BLOCK, partials_off);
    launch("stencil_pipe7", k_stencil_pipe7, blocks, stream, plane_nodes, gx, z0,
           z1, gz, border_base, nown_nodes, pb, diag, wxm, wxp, wym, wyp, wzm, wzp,
           w_old, qpart, z, t, p, xv, r, w_new, scal, first, partials,
           partials_off);
    return blocks;
}

void stencil_spmv(long nrows_nodes, long row0_node, int gx, int gy, int gz,
                  long nown_nodes, uintptr_t zs_of_plane, uintptr_t pb,
                  uintptr_t offs, int ksten, double diag, uintptr_t x,
                  uintptr_t y, bool mato, uintptr_t partials, uintptr_t scal,
                  int dotslot, bool dot_accum, uintptr_t stream) {
    if (nrows_nodes == 0) return;
    const long blocks = elem_grid(nrows_nodes);
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_bool(mato, fuse, [&](auto mo, auto fd) {
        launch("stencil_spmv", k_stencil_spmv<mo, fd>, blocks, stream, nrows_nodes,
               row0_node, gx, gy, gz, nown_nodes, zs_of_plane, pb, offs, ksten,
               diag, x, y, partials);
    });
    if (fuse)
        reduce_partials(partials, (int)blocks, scal, dotslot, dot_accum, stream);
}

long stencil_pipe(long nrows_nodes, long row0_node, long border_base,
                  int gx, int gy, int gz, long nown_nodes,
                  uintptr_t zs_of_plane, uintptr_t pb, uintptr_t offs,
                  int ksten, double diag, uintptr_t w_old, uintptr_t qpart,
                  uintptr_t z, uintptr_t t, uintptr_t p, uintptr_t xv,
                  uintptr_t r, uintptr_t w_new, uintptr_t scal, int first,
                  uintptr_t partials, long partials_off, bool mato,
                  uintptr_t stream) {
    if (nrows_nodes == 0) return 0;
    const long blocks = pipe_grid(elem_grid(nrows_nodes), partials_off);
    dispatch_bool(mato, [&](auto mo) {
        launch("stencil_pipe", k_stencil_pipe<mo>, blocks, stream, nrows_nodes,
               row0_node, border_base, gx, gy, gz, nown_nodes, zs_of_plane, pb,
               offs, ksten, diag, w_old, qpart, z, t, p, xv, r, w_new, scal, first,
               partials, partials_off);
    });
    return blocks;
}

// -- scalars, dots and the fused CG updates -----------------------------------

void pipelined_replace_finalize(uintptr_t partials, int nblocks, uintptr_t scal,
                                uintptr_t stream) {
    launch("pipelined_replace_finalize", k_pipelined_replace_finalize, 1, stream,
           partials, nblocks, scal);
}

void zero_scalars(uintptr_t scal, int i0, int count, uintptr_t stream) {
    launch("zero_scalars", k_zero_scalars, 1, stream, scal, i0, count);
}

void cg_prep_pt(uintptr_t scal, uintptr_t stream) {
    launch_cfg("cg_prep_pt", k_cg_prep_pt, dim3(1), dim3(64), 0, stream, scal);
}

void cg_prep_rr(uintptr_t scal, uintptr_t stream) {
    launch_cfg("cg_prep_rr", k_cg_prep_rr, dim3(1), dim3(64), 0, stream, scal);
}

void dot(uintptr_t x, uintptr_t y, long n, uintptr_t partials, uintptr_t scal,
         int slot, bool accumulate, uintptr_t stream) {
    const long blocks = elem_grid(n);
    launch("dot", k_dot, blocks, stream, x, y, n, partials);
    reduce_partials(partials, (int)blocks, scal, slot, accumulate, stream);
}

void dot2(uintptr_t r, uintptr_t w, long n, uintptr_t partials, uintptr_t scal,
          bool accumulate, uintptr_t stream) {
    const long blocks = elem_grid(n);
    launch("dot2", k_dot2, blocks, stream, r, w, n, partials);
    launch("dot2", k_reduce_partials2, 1, stream, partials, (int)blocks, scal,
           accumulate ? 1 : 0);
}

void axpy_ratio(uintptr_t y, uintptr_t x, long n, uintptr_t scal, int num, int den,
                double sign, uintptr_t stream) {
    launch("axpy_ratio", k_axpy_ratio, elem_grid(n), stream, y, x, n, scal, num,
           den, sign);
}

void daypx_ratio(uintptr_t y, uintptr_t x, long n, uintptr_t scal, int num, int den,
                 uintptr_t stream) {
    launch("daypx_ratio", k_daypx_ratio, elem_grid(n), stream, y, x, n, scal, num,
           den);
}

void pcg_fused_update(uintptr_t r, uintptr_t x, uintptr_t p, uintptr_t t,
                      uintptr_t z, uintptr_t dinv, long n, uintptr_t scal,
                      uintptr_t partials, uintptr_t stream) {
    const long blocks = elem_grid(n);
    launch("pcg_fused_update", k_pcg_fused_update, blocks, stream, r, x, p, t, z,
           dinv, n, scal, partials);
    launch("pcg_fused_update", k_pcg_finalize, 1, stream, partials, (int)blocks,
           scal);
}

void cg_fused_update(uintptr_t r, uintptr_t x, uintptr_t p, uintptr_t t, long n,
                     uintptr_t scal, uintptr_t partials, uintptr_t stream) {
    const long blocks = elem_grid(n);
    launch("cg_fused_update", k_cg_fused_update, blocks, stream, r, x, p, t, n,
           scal, partials);
    launch("cg_fused_update", k_cg_finalize, 1, stream, partials, (int)blocks, scal);
}

long sell_pipe(long nslices, long nrows_pass, long rowbase, long border_base,
               uintptr_t sellptr, uintptr_t cols, uintptr_t vals,
               uintptr_t w_old, uintptr_t qpart, uintptr_t z, uintptr_t t,
               uintptr_t p, uintptr_t x, uintptr_t r, uintptr_t w_new,
               uintptr_t scal, int first, uintptr_t partials,
               long partials_off, bool mato, uintptr_t stream) {
    if (nrows_pass == 0) return 0;
    const long blocks = pipe_grid((nslices * WAVE + BLOCK - 1) / BLOCK, partials_off);
    dispatch_bool(mato, [&](auto mo) {
        launch("sell_pipe", k_sell_pipe<int, true, 8, mo>, blocks, stream, nslices,
               nrows_pass, rowbase, border_base, sellptr, cols, vals, w_old, qpart,
               z, t, p, x, r, w_new, scal, first, partials, partials_off);
    });
    return blocks;
}

void pipelined_finalize(uintptr_t partials, int nblocks, uintptr_t scal, int first,
                        uintptr_t stream) {
    launch("pipelined_finalize", k_pipelined_finalize, 1, stream, partials, nblocks,
           scal, first);
}

void pipelined_fused(uintptr_t z, uintptr_t t, uintptr_t p, uintptr_t x, uintptr_t r,
                     uintptr_t w, uintptr_t q, long n, uintptr_t scal, int first,
                     uintptr_t partials, bool nt_update, uintptr_t stream) {
    const long blocks = elem_grid(n);
    dispatch_bool(nt_update, [&](auto ntu) {
        launch("pipelined_fused", k_pipelined_fused<ntu>, blocks, stream, z, t, p,
               x, r, w, q, n, scal, first, partials);
    });
    pipelined_finalize(partials, (int)blocks, scal, first, stream);
}

// cooperative launch of the monolithic device CG (reference
// acgsolverhip_solve_device geometry logic, cg-kernels-hip.hip:1892-1909:
// grid = CUs x occupancy, everything grid-stride inside)
int cg_device(long nslices, long nrows, uintptr_t sellptr, uintptr_t cols,
              int col64, uintptr_t vals, uintptr_t b, uintptr_t x, uintptr_t r,
              uintptr_t p, uintptr_t t, uintptr_t scal, uintptr_t partials,
              uintptr_t out2, uintptr_t barrier_state,
              int maxits, double res_atol, double res_rtol,
              uintptr_t stream, int hier) {
    int dev = 0;
    hipGetDevice(&dev);
    hipDeviceProp_t props;
    hipGetDeviceProperties(&props, dev);
    const void* kern = col64 ? (const void*)&k_cg_device<long>
                             : (const void*)&k_cg_device<int>;
    int blocks_per_cu = 0;
    hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &blocks_per_cu, kern, BLOCK, 0);
    if (oe != hipSuccess || blocks_per_cu < 1) blocks_per_cu = 1;
    // the occupancy API can over-report by one block/CU and the cooperative
    // launch validates against the same (wrong) number -- a non-resident
    // block would deadlock the grid barrier.  Guide guidance: <= 4 blocks
    // of 256 threads per CU is reliably resident.
    if (blocks_per_cu > 4) blocks_per_cu = 4;
    long grid = (long)props.multiProcessorCount * blocks_per_cu;
    long need = (nslices * WAVE + BLOCK - 1) / BLOCK;
    if (grid > need) grid = need;
    if (grid > MAXG) grid = MAXG;
    // hier < 0 = auto: per-XCD staging pays beyond ~64 blocks (measured
    // MI355X: 1024 blocks flat 192 us/it vs hier 76; 16 blocks flat
    // 15.6 vs 18.7 -- tools/devcg_barrier_ab.py)
    if (hier < 0) hier = grid >= 64 ? 1 : 0;
    // the occupancy API can over-report by one block/CU (guide §1); the
    // cooperative launch checks residency -- shrink and retry on rejection.
    for (;;) {
        void* args[] = {&nslices, &nrows, (void*)&sellptr, (void*)&cols,
                        (void*)&vals, (void*)&b, (void*)&x, (void*)&r,
                        (void*)&p, (void*)&t, (void*)&scal, (void*)&partials,
                        (void*)&out2, (void*)&barrier_state,
                        &maxits, &res_atol, &res_rtol, &hier};
        hipError_t e = hipLaunchCooperativeKernel(
            kern, dim3((unsigned)grid), dim3(BLOCK), args, 0, S(stream));
        if (e == hipSuccess) break;
        if (e == hipErrorCooperativeLaunchTooLarge && grid > props.multiProcessorCount) {
            (void)hipGetLastError();
            grid -= props.multiProcessorCount;
            continue;
        }
        throw std::runtime_error(std::string("cg_device launch: ") + hipGetErrorString(e));
    }
    check_hip("cg_device");
    return (int)grid;
}

void atomic_probe(uintptr_t y, uintptr_t idx, uintptr_t v, long nnz,
                  int mode, uintptr_t stream) {
    launch("atomic_probe", k_atomic_probe, elem_grid(nnz, 8), stream, y, idx, v,
           nnz, mode);
}

void pack_gather(uintptr_t sendbuf, uintptr_t x, uintptr_t idx, int idx64, long n,
                 uintptr_t stream) {
    if (n == 0) return;
    dispatch_index(idx64, [&](auto it) {
        using IT = typename decltype(it)::type;
        launch("pack_gather", k_pack_gather<IT>, elem_grid(n, 1), stream, sendbuf,
               x, idx, n);
    });
}

// -- multiple right-hand sides ------------------------------------------------

void reduce_partials_multi(uintptr_t partials, int nblocks, int k, uintptr_t scal,
                           int slot, bool accumulate, uintptr_t stream) {
    if (k < 1 || k > 8) throw std::invalid_argument("reduce_partials_multi: K must be 1..8");
    if (nblocks < 0 || nblocks > MAXG || slot < 0 || slot >= S_NSLOTS)
        throw std::invalid_argument("reduce_partials_multi: nblocks/slot out of range");
    launch("reduce_partials_multi", k_reduce_partials_multi, k, stream, partials,
           nblocks, scal, slot, accumulate ? 1 : 0);
}

long spmm_sell(long nslices, long nrows, int k, uintptr_t sellptr, uintptr_t cols,
               int col64, uintptr_t vals, uintptr_t X, uintptr_t Y,
               uintptr_t partials, uintptr_t scal, int dotslot, bool dot_accum,
               uintptr_t perm, uintptr_t stream) {
    if (nrows == 0 || nslices == 0) return 0;
    const long blocks = slice_grid(nslices);
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_k(k, "spmm_sell", [&](auto kk) {
        constexpr int KK = kk;
        dispatch_index(col64, [&](auto ct) {
            using CT = typename decltype(ct)::type;
            dispatch_bool(fuse, perm != 0, [&](auto fd, auto pm) {
                launch("spmm_sell", k_spmm_sell<CT, KK, fd, pm>, blocks, stream,
                       nslices, nrows, sellptr, cols, vals, X, Y, partials, perm);
            });
        });
    });
    if (fuse)
        reduce_partials_multi(partials, (int)blocks, k, scal, dotslot, dot_accum, stream);
    return blocks;
}

// (dof, K) pairs with a register-resident instantiation; none spills, so
// every pair is offered (see profiles/multi_rhs.md for the table)
bool spmm_bsell_supported(int dof, int k) {
    return dof >= 2 && dof <= 4 && (k == 2 || k == 4 || k == 8);
}

long spmm_bsell(long nslices, long nnodes, int dof, int k, uintptr_t bptr,
                uintptr_t bcol, uintptr_t bvals, uintptr_t X, uintptr_t Y,
                uintptr_t partials, uintptr_t scal, int dotslot, bool dot_accum,
                uintptr_t stream) {
    if (!spmm_bsell_supported(dof, k))
        throw std::invalid_argument("spmm_bsell: dof must be 2/3/4 and K 2/4/8");
    if (nnodes == 0 || nslices == 0) return 0;
    const long blocks = slice_grid(nslices);
    const bool fuse = partials != 0 && dotslot >= 0;
    dispatch_k(k, "spmm_bsell", [&](auto kk) {
        constexpr int KK = kk;
        dispatch_dof(dof, "spmm_bsell", [&](auto d) {
            constexpr int D = d;
            dispatch_bool(fuse, [&](auto fd) {
                launch("spmm_bsell", k_spmm_bsell<D, KK, fd>, blocks, stream,
                       nslices, nnodes, bptr, bcol, bvals, X, Y, partials);
            });
        });
    });
    if (fuse)
        reduce_partials_multi(partials, (int)blocks, k, scal, dotslot, dot_accum, stream);
    return blocks;
}

long dot_multi(uintptr_t X, uintptr_t Y, long n, int k, uintptr_t partials,
               uintptr_t scal, int slot, bool accumulate, uintptr_t stream) {
    const long blocks = elem_grid(n * k / 2, 1);
    dispatch_k(k, "dot_multi", [&](auto kk) {
        launch("dot_multi", k_dot_multi<kk>, blocks, stream, X, Y, n * kk / 2,
               partials);
    });
    reduce_partials_multi(partials, (int)blocks, k, scal, slot, accumulate, stream);
    return blocks;
}

// update only: the K partial sets stay in `partials` for cg_finalize_multi;
// returns the number of blocks (= partials per column)
long cg_fused_update_multi(uintptr_t R, uintptr_t X, uintptr_t P, uintptr_t T,
                           long n, int k, uintptr_t scal, uintptr_t partials,
                           uintptr_t stream) {
    const long blocks = elem_grid(n * k / 2, 1);
    dispatch_k(k, "cg_fused_update_multi", [&](auto kk) {
        launch("cg_fused_update_multi", k_cg_fused_update_multi<kk>, blocks, stream,
               R, X, P, T, n * kk / 2, scal, partials);
    });
    return blocks;
}

void cg_finalize_multi(uintptr_t partials, int nblocks, int k, uintptr_t scal,
                       uintptr_t rr_out, uintptr_t stream) {
    if (k < 1 || k > 8) throw std::invalid_argument("cg_finalize_multi: K must be 1..8");
    if (nblocks < 0 || nblocks > MAXG)
        throw std::invalid_argument("cg_finalize_multi: nblocks out of range");
    launch("cg_finalize_multi", k_cg_finalize_multi, k, stream, partials, nblocks,
           scal, rr_out);
}

void daypx_ratio_multi(uintptr_t P, uintptr_t R, long n, int k, uintptr_t scal,
                       int num, int den, uintptr_t stream) {
    if (num < 0 || num >= S_NSLOTS || den < 0 || den >= S_NSLOTS)
        throw std::invalid_argument("daypx_ratio_multi: slot out of range");
    const long blocks = elem_grid(n * k / 2, 1);
    dispatch_k(k, "daypx_ratio_multi", [&](auto kk) {
        launch("daypx_ratio_multi", k_daypx_ratio_multi<kk>, blocks, stream, P, R,
               n * kk / 2, scal, num, den);
    });
}

// -- block CG -------------------------------------------------------------------

static void block_check(const char* what, int k, int kg, int nblocks) {
    if (k != 2 && k != 4 && k != 8)
        throw std::invalid_argument(std::string(what) + ": K must be 2, 4 or 8");
    if (kg < 1 || kg > k)
        throw std::invalid_argument(std::string(what) + ": kg must be in 1..K");
    if (nblocks < 1 || nblocks > BLOCK_MAXG)
        throw std::invalid_argument(std::string(what) + ": nblocks out of range");
}

// returns the number of blocks (= partials per pair)
long gram_multi(uintptr_t X, uintptr_t Y, long n, int k, uintptr_t partials,
                uintptr_t stream) {
    const long blocks = block_grid(n);
    dispatch_k(k, "gram_multi", [&](auto kk) {
        launch("gram_multi", k_gram_multi<kk>, blocks, stream, X, Y, n, partials);
    });
    return blocks;
}

long block_update(uintptr_t X, uintptr_t Sm, uintptr_t Q, uintptr_t T, long n, int k,
                  uintptr_t state, uintptr_t partials, uintptr_t stream) {
    const long blocks = block_grid(n);
    dispatch_k(k, "block_update", [&](auto kk) {
        launch("block_update", k_block_update<kk>, blocks, stream, X, Sm, Q, T, n,
               state, partials);
    });
    return blocks;
}

void block_ortho(uintptr_t Q, uintptr_t Sm, long n, int k, uintptr_t state,
                 uintptr_t stream) {
    dispatch_k(k, "block_ortho", [&](auto kk) {
        launch("block_ortho", k_block_ortho<kk>, block_grid(n), stream, Q, Sm, n,
               state);
    });
}

void block_coef_alpha(uintptr_t partials, int nblocks, uintptr_t state, int k,
                      int kg, int it, uintptr_t stream) {
    block_check("block_coef_alpha", k, kg, nblocks);
    launch("block_coef_alpha", k_block_coef_alpha, 1, stream, partials, nblocks,
           state, k, kg, it);
}

void block_coef_beta(uintptr_t partials, int nblocks, uintptr_t state,
                     uintptr_t rr_out, int k, int kg, int it, bool init,
                     uintptr_t stream) {
    block_check("block_coef_beta", k, kg, nblocks);
    launch("block_coef_beta", k_block_coef_beta, 1, stream, partials, nblocks,
           state, rr_out, k, kg, it, init ? 1 : 0);
}

PYBIND11_MODULE(_acg_kernels, m) {
    m.doc() = "acg_amd gfx950 HIP kernels";
    m.def("spmm_sell", &spmm_sell);
    m.def("spmm_bsell", &spmm_bsell);
    m.def("spmm_bsell_supported", &spmm_bsell_supported);
    m.def("dot_multi", &dot_multi);
    m.def("reduce_partials_multi", &reduce_partials_multi);
    m.def("cg_fused_update_multi", &cg_fused_update_multi);
    m.def("cg_finalize_multi", &cg_finalize_multi);
    m.def("daypx_ratio_multi", &daypx_ratio_multi);
    m.def("gram_multi", &gram_multi);
    m.def("block_update", &block_update);
    m.def("block_ortho", &block_ortho);
    m.def("block_coef_alpha", &block_coef_alpha);
    m.def("block_coef_beta", &block_coef_beta);
    m.attr("BS_LD") = BS_LD;
    m.attr("BS_M") = BS_M;
    m.attr("BS_XI") = BS_XI;
    m.attr("BS_XIC") = BS_XIC;
    m.attr("BS_G") = BS_G;
    m.attr("BS_ZETA") = BS_ZETA;
    m.attr("BS_ZINV") = BS_ZINV;
    m.attr("BS_C") = BS_C;
    m.attr("BS_FLAG") = BS_FLAG;
    m.attr("BS_ITER") = BS_ITER;
    m.attr("BS_SIZE") = BS_SIZE;
    m.attr("BLOCK_MAXG") = BLOCK_MAXG;
    m.attr("BLOCK_TAU") = BLOCK_TAU;
    m.def("spmv", &spmv);
    m.def("spmv_binned", &spmv_binned);
    m.def("spmv_sell", &spmv_sell);
    m.attr("SELL_NT") = SELL_NT;
    m.attr("SELL_SWZ") = SELL_SWZ;
    m.attr("SELL_U8") = SELL_U8;
    m.def("spmv2_sell", &spmv2_sell);
    m.def("zero_scalars", &zero_scalars);
    m.def("cg_prep_pt", &cg_prep_pt);
    m.def("cg_prep_rr", &cg_prep_rr);
    m.def("dot", &dot);
    m.def("dot2", &dot2);
    m.def("axpy_ratio", &axpy_ratio);
    m.def("daypx_ratio", &daypx_ratio);
    m.def("cg_fused_update", &cg_fused_update);
    m.def("pcg_fused_update", &pcg_fused_update);
    m.def("bsell_diag_inv", &bsell_diag_inv);
    m.def("bjacobi_apply", &bjacobi_apply);
    m.def("bpcg_fused_update", &bpcg_fused_update);
    m.def("pipelined_fused", &pipelined_fused);
    m.def("sell_pipe", &sell_pipe);
    m.def("pipelined_finalize", &pipelined_finalize);
    m.def("pipelined_replace_finalize", &pipelined_replace_finalize);
    m.def("dot2_slices", &dot2_slices);
    m.def("pack_gather", &pack_gather);
    m.def("atomic_probe", &atomic_probe);
    m.def("cg_device", &cg_device);
    m.attr("BAR_STATE_WORDS") = BAR_STATE_WORDS;
    m.def("stencil_rowlen", &stencil_rowlen);
    m.def("stencil_fill", &stencil_fill);
    m.def("spmv_bsell", &spmv_bsell);
    m.def("spmv2_bsell", &spmv2_bsell);
    m.def("spmv_bsell_daypx", &spmv_bsell_daypx);
    m.def("spmv_bsell_st", &spmv_bsell_st);
    m.attr("ST_NOSEND") = ST_NOSEND;
    m.attr("ST_TILE") = BLOCK;  // nodes per BSELL-ST tile = one workgroup
    m.def("stencil_blocklen", &stencil_blocklen);
    m.def("stencil_bfill", &stencil_bfill);
    m.def("stencil_spmv", &stencil_spmv);
    m.def("stencil_pipe", &stencil_pipe);
    m.def("stencil_spmv7", &stencil_spmv7);
    m.def("stencil_pipe7", &stencil_pipe7);
    m.attr("S_RR") = S_RR;
    m.attr("S_PT") = S_PT;
    m.attr("S_RR_PREV") = S_RR_PREV;
    m.attr("S_BNRM2") = S_BNRM2;
    m.attr("S_GAMMA") = S_GAMMA;
    m.attr("S_DELTA") = S_DELTA;
    m.attr("S_GAMMA_PREV") = S_GAMMA_PREV;
    m.attr("S_ALPHA_PREV") = S_ALPHA_PREV;
    m.attr("S_NSLOTS") = S_NSLOTS;
    m.attr("MAXG") = MAXG;
}

