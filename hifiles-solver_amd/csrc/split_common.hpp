// split_common.hpp -- tables, element geometry and device helpers shared by the split fused kernels, and the plan of a split
// stage (SplitPlan).  The kernels themselves (split2_kernels.hpp, split3_kernels.hpp) are included by fused_hex.hip only -- one
// translation unit, so that every kernel is instantiated once; comm.hip and deferred.hip read the plan.
#pragma once
#include <memory>
#include <vector>

#include "fused_hex.hpp"
#include "physics.hpp"

namespace hfx
{

constexpr int MAX_TAB = 256;

// minimum waves per SIMD the residual kernel of fused = 2 is compiled for (second __launch_bounds__ argument)
#ifndef HFX_SPLIT_WAVES_RES
#define HFX_SPLIT_WAVES_RES 4
#endif

struct FusedData
{
  DevBuf<unsigned char> meta; // bit0: this point is the RIGHT side, bit1: beta sign flipped, bit2: boundary point
  DevBuf<double> disu_alt;    // second disu_fpts buffer
  DevBuf<double> fn_fpts;     // split variant 3: projected viscous flux per flux point (n_fpts,n_eles,n_fields)
  // tensor-product tables of the sum-factorised flux kernel (valid when tensor_ok)
  DevBuf<long long> stamps; // diagnostics buffer (HFX_FLUX_STAMPS=1)
  bool tensor_ok = false;
  DevBuf<double> t_coef; // Dm[N][N] | c5[ND][2][N] | Lf[ND][2][N] | L1[ND][2][N] | c3[ND][2][N]
  std::vector<double> h_coef; // host copy
  DevBuf<int> t_idx;     // pf[ND][L][2] | fdq[NFP] | fbase[NFP]
  DevBuf<unsigned> pk_g, pk_r; // packed operator rows of the gradient / residual kernel
  DevBuf<double> tab_g, tab_r; // value tables (MAX_TAB doubles)
  DevBuf<int> o1m_dim;                       // (n_fpts) dimension slab of the merged opp_1 row
  DevBuf<int> nbr;                           // (n_fpts, n_eles) partner of every interior flux point (split3_kernels.hpp, Split2Args::nbr)
  long n_interior_fpts = 0;                  // flux points with a partner in a registered interior face (two per pair)
  // partitioned blocks: the elements that own a flux point without a registered face (= a partition-face point), and the rest
  DevBuf<int> upd_list_b, upd_list_i;
  long n_list_b = 0, n_list_i = 0;
  long n_list_i1 = 0; // the flux kernel takes the others in two parts: upd_list_i[0 .. n_list_i1) and the rest
  DevBuf<double> les_len2;                   // (n_upts, n_eles) squared length scale of the LES closure evaluated in the flux kernel
  // an AFFINE block (every element a parallelepiped: metrics constant inside an element up to the rounding of their own
  // evaluation -- affine_detect, fused_hex.hip): one AffRec per element in place of the per-point metric arrays
  bool affine = false;
  double affine_tol = 0.0, affine_spread = 0.0; // the relative bound of the test and the largest spread it met (diagnostics)
  DevBuf<double> aff_rec;                       // (AffRec::SIZE, n_eles)
  // two-wave flux kernel (split_flux_two_wave_kernel): per local face, the elements by what the face's first n_fpts - 128 points
  // (the left-over points, were the face chosen) ask of their projected viscous flux -- bit0: a point without a partner word
  // (always needed), bit1: a point needed unless ldg_beta = -1/2, bit2: a point needed unless ldg_beta = +1/2 (two_wave_face)
  long tw_need[6][8] = {};
  bool tw_counted = false;
  bool built = false;
};

// The metric record of one element of an affine block (the face's tdA is recorded, no kernel reads it yet), 34 doubles (quads use the first 26): JGinv (n_dims^2, as in JGinv_upts),
// detjac, then per local face the own normal (n_dims of 3 slots) and tdA.  Element stride 272 bytes and face offset 80 + 32 f:
// a record is 17 16-byte lanes of the loader wave's LDS-DMA, a face is one aligned 32-byte read.
struct AffRec
{
  static constexpr int JG = 0, DJ = 9, FACE = 10, FACE_W = 4, TDA = 3, SIZE = 34;
};

// the flux kernel of variant 3: the loader-wave form of split_flux_tensor_kernel, its register-pipeline forms, or the
// dictionary-row kernel split_flux_kernel
enum class FluxForm { loader_wave, register_pipeline, dictionary_rows };
// where the de-aliased flux of over-integration comes from: the sum-factorised kernel's result folded into the divergence, the
// same kernel's tdisf_upts, or the dense contraction
enum class OverInt { none, folded_tensor, tensor, dense };

// What the split fused stage runs on one block for one request (split_plan, fused_hex.hip): every form decided once, from the
// options, the block's fused tables, its flags and its array sizes.  Launch geometry (grids, element order, SIMD roles) is not
// part of it.
struct SplitPlan
{
  int variant = 2;              // the variant that runs (a request for 3 falls back to 2)
  bool les_in_flux = false;     // the LES closure is evaluated in the flux kernel of variant 3
  // the four "every array below 4 GiB" tests, each with its own count of the largest array
  bool les_fits_4gib = false;
  bool gather_fits_4gib = false;
  bool flux_buf_fits_4gib = false;
  bool update_fits_4gib = false;
  // variant 3
  FluxForm flux = FluxForm::dictionary_rows;
  bool oi = false, les = false; // loader wave: the OI / LES flags (GA = gather); register pipeline: OI
  int wv = 2;                   // register pipeline: WV
  bool buf = false;             // register pipeline: BUF
  bool gather = false;          // the flux kernel forms the interior LDG corrections itself (loader wave: GA)
  bool affine = false;          // an affine block: the flux kernel (loader wave: AFF) and the update kernel read the per-element metric record
  bool two_wave = false;        // the affine flux kernel in its two-wave form (split_flux_two_wave_kernel: P4 hexahedra, option flux_two_wave)
  bool fold_faces = false;      // the two-wave flux kernel forms the interior pairs' common flux (its FOLD form: viscous, |ldg_beta| = 1/2, not RoeM, option fold_faces) and no face_flux2_kernel is launched on the interior faces
  bool face_delta = false;      // face_delta_kernel forms them (a viscous block without `gather`)
  bool oi_fold = false;         // the over-integration kernel hands over its result folded into the divergence
  OverInt over_int = OverInt::none;
  bool update_buf = false;      // split_update_kernel with buffer addressing
  bool bdy_grad = false;        // the flux kernel stores the gradient at the boundary points (a viscous block with boundary faces)
  // a partitioned block: the projected viscous flux on the wire; the flux kernel / the update on element lists may run
  bool projected = false, split_flux = false, split_update = false;
  // hfx_time_fused_kernels: the stage's four kernels, and what part 2 adds (the over-integration kernel, the SGS kernels)
  const char *names = "", *extra_names = "";
};

// The elements a launch of the flux or update kernel works on: all, or one of a partitioned block's lists (FusedData)
enum class EleList
{
  all,
  interior_1, // the first part of the elements without partition-face points: upd_list_i[0 .. n_list_i1)
  partition,  // the elements with partition-face points: upd_list_b
  interior_2, // the rest of upd_list_i
  interior,   // upd_list_i
};

// ONE RK stage of the split path on one block whose fused tables exist (ensure_fused_tables), as named steps on the compute
// stream.  make() does once what every step relies on: the element size's implementation (fused_hex.hip), the kernel arguments
// of the variant that runs, the face arguments, the allocations of variant 3 (fn_fpts, stamps, les_len2) and the folded
// over-integration matrices.  The arguments name the disu_fpts buffers as they are when the stage is made, and update()
// exchanges them: a SplitStage is made before the stage's first launch and does not outlive the stage.
struct SplitStage
{
  hfx_eles *const e;
  hfx_inters *const *const faces;
  const int nfb;
  const SplitPlan pl;
  // write_div: store div_tconf_upts (the last stage of a step).  Null: error (message in hfx_last_error)
  static std::unique_ptr<SplitStage> make(hfx_eles *e, hfx_inters *const *faces, int nfb, int in_step, bool write_div, const SplitPlan &pl);
  virtual ~SplitStage() = default;
  // viscous: the ghost states of the boundary faces (-> inviscid common flux, LDG common solution); face_delta_kernel where
  // the plan says so (pl.face_delta)
  virtual int ldg() = 0;
  // variant 3: the over-integration kernel where the block de-aliases; the flux kernel, on a partitioned block in up to three
  // launches (interior_1 needs nothing from the neighbours; an empty list launches nothing)
  int over_int();
  virtual int flux_kernel(EleList list = EleList::all) = 0;
  // variant 2, viscous: the gradient kernel; with an LES closure the SGS flux at the solution points and its extrapolation
  virtual int gradient_kernel() = 0;
  int sgs_kernels();
  // everything element-local between the two cuts of the stage, for the variant that runs
  // (over-integration works on all elements: a list with it is refused by flux_kernel, before anything is launched)
  int element_kernels(EleList list = EleList::all) { return pl.variant == 3 ? (list == EleList::all && over_int()) || flux_kernel(list) : gradient_kernel() || sgs_kernels(); }
  // the viscous fluxes of the boundary faces (option bdy_beside: on the side stream) and the pairwise common-flux kernel
  virtual int common_fluxes() = 0;
  // the update (variant 3) | residual (variant 2) kernel: RK update and the NEW state's flux-point solution, written to the
  // second disu_fpts buffer.  The buffers change places behind the first update launch of a stage (all | partition), so
  // `interior`, which follows `partition`, writes the buffer that is disu_fpts by then.  An empty list launches nothing.
  virtual int update(EleList list = EleList::all) = 0;
  int run() { return ldg() || element_kernels() || common_fluxes() || update(); }
protected:
  SplitStage(hfx_eles *e_, hfx_inters *const *faces_, int nfb_, const SplitPlan &pl_) : e(e_), faces(faces_), nfb(nfb_), pl(pl_) {}
  virtual int init(int in_step, bool write_div) = 0;
  // the list's elements (false: `all`)
  bool elements(EleList list, const int *&ele_list, long &n_list) const;
};

// ONE stage of the split fused path on a PARTITIONED block (split_partitioned.hpp): a SplitStage for the elements and the
// interior and boundary faces, and the steps at the partition faces.  init() does once what every step relies on: argument
// checks, the block's fused tables, the plan, the stage range, the stage.  Which steps a stage takes is the caller's choice from
// the plan (stage->pl: variant, projected, split_flux, split_update) and from `viscous`.  st: the stream of the one-sided
// partition-face kernels; everything else runs on the context's compute stream.  The steps of a viscous stage, in order:
//   [pack_solution]  interior_ldg  partition_ldg  stage->element_kernels  pack_projected_flux | pack_gradient [pack_sgs_flux]
//   stage->common_fluxes  partition_common_fluxes | partition_common_invflux, partition_common_viscflux  update  pack_solution
struct PartitionedSplit
{
  hfx_eles *e = nullptr;
  hfx_inters *const *mpi_faces = nullptr;
  int n_mpi = 0, in_step = 0;
  std::unique_ptr<SplitStage> stage;
  int init(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi, int in_step);
  int pack_solution(hipStream_t st) const { return mpi_all(MpiKernel::pack_solution, st); }
  // viscous: the LDG common solution at the boundary and interior faces (at the first stage behind the Leonard terms of an LES
  // closure; the SVV closure is refused: it filters a state whose flux-point values have left already) | at the partition faces
  int interior_ldg() const;
  int partition_ldg(hipStream_t st) const { return mpi_all(MpiKernel::ldg_delta, st); }
  // the second message: variant 3 the projected viscous flux (behind the element kernel) | variant 2 the corrected gradient
  // and, with an LES closure, a third message: the physical SGS flux (src/solver.cpp:168-178)
  int pack_projected_flux(hipStream_t st) const { return mpi_all(MpiKernel::pack_projected_flux, st); }
  int pack_gradient(hipStream_t st) const { return mpi_all(MpiKernel::pack_gradient, st); }
  int pack_sgs_flux(hipStream_t st) const { return mpi_all(MpiKernel::pack_sgs_flux, st); }
  // the common fluxes at the partition faces: variant 3 from both sides' solution and projected flux; variant 2 the inviscid
  // part (needs the solution only) and, viscous, the part from the gradients
  int partition_common_fluxes(hipStream_t st) const { return mpi_all(MpiKernel::common_flux_projected, st); }
  int partition_common_invflux(hipStream_t st) const { return mpi_all(MpiKernel::common_invflux, st); }
  int partition_common_viscflux(hipStream_t st) const { return mpi_all(MpiKernel::common_viscflux, st); }
  // the stage's update, whole (then shock capturing where the block has it) or with pl.split_update in two launches: `partition`
  // (whose new flux-point solution can then leave) and `interior`
  int update(EleList list = EleList::all) const;
private:
  int mpi_all(MpiKernel k, hipStream_t st) const; // kernel k on every partition-face block
};

constexpr int ipow(int b, int e) { return e == 0 ? 1 : b * ipow(b, e - 1); }
// 32-bit words that hold `w` packed row entries, `epw` entries per word
constexpr int words_of(int w, int epw = 2) { return (w + epw - 1) / epw; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int ND, int N>
struct Geo
{
  static constexpr int NF = ND + 2;
  static constexpr int NU = ipow(N, ND);
  static constexpr int NFP = 2 * ND * ipow(N, ND - 1);
  static constexpr int WU = (NU + 63) / 64;  // solution-point waves
  static constexpr int WF = (NFP + 63) / 64; // flux-point waves
  static constexpr int TU = 64 * WU;
  static constexpr int TB = 64 * (WU + WF);       // gradient kernel: roles U, F
  static constexpr int TBR = 64 * (WU + 2 * WF);  // residual kernel: roles U, A, B
  static constexpr int UNP = (NF * NU + TU - 1) / TU; // doubles of the next element's state per upt thread
  // A packed row entry is 16 bits (8-bit value id | 8-bit column), two per word, while every column fits 8 bits.  Hexes
  // from P6 on (343 / 512 solution points) take WIDE entries: value id << 16 | 16-bit column, one per word.
  static constexpr bool WIDE = NU > 256 || NFP > 256;
  static constexpr int EPW = WIDE ? 1 : 2;       // entries per word
  static constexpr int WN = words_of(N, EPW);     // words of an N-entry row
  static constexpr int W2 = words_of(2, EPW);     // words of an opp_5 row
  static constexpr int W3 = words_of(2 * ND, EPW); // words of an opp_3 row
  // packed-row layout, gradient kernel: opp_4[d] | opp_5[d] (rows = upts) | opp_0 | opp_6 (rows = fpts)
  static constexpr int G_O4 = 0;
  static constexpr int G_O5 = G_O4 + ND * WN * NU;
  static constexpr int G_O0 = G_O5 + ND * W2 * NU;
  static constexpr int G_O6 = G_O0 + WN * NFP;
  static constexpr int G_END = G_O6 + WN * NFP;
  static constexpr int G_WU = ND * WN + ND * W2; // words per upt thread
  static constexpr int G_WF = 2 * WN;                     // words per fpt thread
  // residual kernel: opp_2[d] | opp_3 (upts) | opp_0 | merged opp_1 (fpts)
  static constexpr int R_O2 = 0;
  static constexpr int R_O3 = R_O2 + ND * WN * NU;
  static constexpr int R_O0 = R_O3 + W3 * NU;
  static constexpr int R_O1 = R_O0 + WN * NFP;
  static constexpr int R_END = R_O1 + WN * NFP;
  static constexpr int R_WU = ND * WN + W3;
  static constexpr int R_WF = 2 * WN;
};

// acc += sum_q tab[vid_q] * data[col_q], ascending q (= ascending column).  `w` is a
// register array subscripted with compile-time constants only.  WIDE: one 32-bit entry per word (Geo::WIDE).
template <int W, int OFF, int PW, bool WIDE = false>
__device__ __forceinline__ double row_dot(const unsigned (&w)[PW], const double *tab, const double *data, double acc)
{
#pragma unroll
  for (int i = 0; i < words_of(W, WIDE ? 1 : 2); i++)
  {
    // The unpacked (value id, column) pairs are loop invariant; left alone the compiler hoists
    // all of them out of the persistent loop and the ~12 packed registers turn back into ~100
    // address registers.  The empty asm makes the word opaque so that it is unpacked at the use.
    unsigned word = w[OFF + i];
    asm volatile("" : "+v"(word));
    if constexpr (WIDE)
      acc += tab[word >> 16] * data[word & 0xffffu];
    else
    {
      {
        const unsigned ent = word & 0xffffu;
        acc += tab[ent >> 8] * data[ent & 0xffu];
      }
      if (2 * i + 1 < W)
      {
        const unsigned ent = word >> 16;
        acc += tab[ent >> 8] * data[ent & 0xffu];
      }
    }
  }
  return acc;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains every outstanding
// GLOBAL load and store of the wave (s_waitcnt vmcnt(0)); the roles exchange data through LDS
// only, so waiting for the LDS counter is sufficient and result stores / prefetches stay in flight.
__device__ __forceinline__ void lds_barrier()
{
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// g_phys(d) = sum_l (inv_detjac * g_ref(l)) * JGinv(l,d)   (BLAS=NO branch of src/eles.cpp:1975-1979)
template <int ND>
__device__ __forceinline__ void to_physical(const double inv_detjac, const double (&JG)[ND * ND], const double (&tg)[ND],
                                            double (&cg)[ND])
{
#pragma unroll
  for (int d = 0; d < ND; d++) cg[d] = 0.0;
#pragma unroll
  for (int l = 0; l < ND; l++)
  {
    const double temp = inv_detjac * tg[l];
#pragma unroll
    for (int d = 0; d < ND; d++) cg[d] += temp * JG[l + ND * d];
  }
}

} // namespace hfx
