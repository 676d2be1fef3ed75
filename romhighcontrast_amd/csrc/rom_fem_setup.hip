// rom_fem_create: plans the FE space on the host (rom_fem_plan.hip: interface layout, compression, symbolic tile Cholesky,
// every parameter-independent table), uploads the tables and runs the three device-side builds (A0, G, Gs).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "rom_fem_dev.h"

// forcing switches of the A/B build (see the end of rom_fem_create); the product build reads none of them
#ifdef ROMHC_AB
static const char* ab_env(const char* name) { return getenv(name); }
#else
static const char* ab_env(const char*) { return nullptr; }
#endif

FemDev make_dev(const rom_fem* f) {
  FemDev d;
  d.nrb = f->nrb; d.ncb = f->ncb; d.N = f->N; d.n1 = f->n1; d.n1p = f->n1p; d.nr = f->nr; d.nc = f->nc;
  d.nGp = f->nGp; d.nGa = f->nGa; d.T = f->T; d.nslots = f->nslots; d.kblk = f->nrb * f->ncb; d.npre = f->npre;
  d.nrhs = f->nrhs; d.nexp = f->nexp; d.ncross = f->ncross; d.xb0 = f->xb0; d.dim = f->dim;
  // tile assembly
  d.pool = f->d_pool; d.alist = f->d_alist; d.aoff = f->d_aoff; d.tile_stream = f->sw_no_tile_stream ? 0 : 1;
  d.pairs = f->d_pairs; d.npairs = f->npairs; d.pool_acc = f->d_pool_acc; d.wmeta = f->d_wmeta;
  for (int i = 0; i < 5; ++i) d.wp0[i] = f->wp0[i];
  d.s1_t0 = d.s1_nterm = d.s1_ndr = 0;
  if (f->fused1 && !f->desc.empty()) {
    d.s1_t0 = f->desc[0].t0; d.s1_nterm = f->desc[0].t1 - f->desc[0].t0; d.s1_ndr = f->desc[0].ndr;
  }
  d.s1_items = f->d_s1_items; d.s1_citems = f->d_s1_citems; d.terms = f->d_terms;
  // closed-form edges, expansion, scalar block
  d.Bt = f->d_Bt; d.P = f->d_P; d.vec = f->d_vec; d.rhs = f->d_rhs; d.pre = f->d_pre; d.exp = f->d_exp;
  d.xred = f->d_xred; d.scb = f->d_scb; d.spos0 = f->spos0; d.nsc = f->nsc; d.sblk0 = f->spos0 + f->n_all_edges;
  // coefficient blocks: dense single-tile path, k_coef
  d.dgroups = f->d_dgroups; d.dweight = f->d_dweight; d.ditem_group = f->d_ditem_group; d.ditem_k = f->d_ditem_k;
  d.dmat = f->d_dmat; d.ndg = f->ndg; d.ndi = f->ndi;
  d.groups = f->d_groups; d.cm = f->d_cm; d.item_group = f->d_item_group; d.item_k = f->d_item_k;
  d.item_cf = f->d_item_cf; d.ctask = f->d_ctask; d.nctask = f->nctask; d.ncf = f->ncf; d.gdots = f->d_dots;
  d.ncoef = f->ncoef;
  // extension
  d.G = f->d_G; d.Gs = f->d_Gs; d.A0 = f->d_A0; d.Qp = f->d_Qp; d.kmax = f->d_kmax; d.epos = f->d_epos;
  d.yhat = f->d_yhat; d.W = f->d_W; d.g = f->d_g;
  // tile Cholesky, block lists, maps, workspace
  d.desc = f->d_desc; d.kptr = f->d_kptr; d.kpair = f->d_kpair; d.colptr = f->d_colptr; d.colrow = f->d_colrow;
  d.colti = f->d_colti; d.sides = f->d_sides; d.n_lr = f->n_lr_blocks; d.lr_blocks = f->d_lr_blocks;
  d.gen_blocks = f->d_gen_blocks; d.vmap = f->d_vmap; d.scat = f->d_scat; d.nscat = f->nscat;
  d.L = f->d_L; d.invL = f->d_invL; d.y = f->d_y; d.status = f->ctx->d_status;
  return d;
}

namespace {

// Device allocations are recorded where they are made: in rom_fem::tables (freed by rom_fem_destroy), or in a TempTables
// for the operands of the device-side builds.
struct TempTables {
  std::vector<void*> list;
  ~TempTables() {
    for (void* p : list) hipFree(p);
  }
};

template <class Tp>
int dev_alloc(std::vector<void*>& owner, Tp** dptr, size_t count) {
  ROM_HIP(hipMalloc(dptr, std::max<size_t>(count, 1) * sizeof(Tp)));
  owner.push_back(*dptr);
  return ROM_OK;
}

// Table uploads go through the context's (non-blocking) compute stream, the stream every reader runs on, and wait for
// it: the host vector may be destroyed on return, and no ordering is left to a null-stream copy being host-synchronous.
template <class Tp>
int upload(hipStream_t st, std::vector<void*>& owner, Tp** dptr, const std::vector<Tp>& h) {
  ROM_TRY(dev_alloc(owner, dptr, h.size()));
  if (!h.empty()) {
    ROM_HIP(hipMemcpyAsync(*dptr, h.data(), h.size() * sizeof(Tp), hipMemcpyHostToDevice, st));
    ROM_HIP(hipStreamSynchronize(st));
  }
  return ROM_OK;
}

// the device-side builds: A0 from the sine matrix and rho, the extension tables G = A0 Bh^T, their segment-major copies Gs
int build_extension_tables(rom_fem* f, const FemPlan& p) {
  rom_ctx* ctx = f->ctx;
  const int n1 = p.n1, n1p = p.n1p;
  const size_t hrows = size_t(n1) * n1;
  ROM_TRY(dev_alloc(f->tables, &f->d_A0, hrows * n1p));
  if (hrows > 0) {
    TempTables tmp;
    double* d_rho = nullptr;
    ROM_TRY(upload(ctx->stream, tmp.list, &d_rho, p.rho));
    k_build_A0<<<unsigned((hrows * n1p + 255) / 256), 256, 0, ctx->stream>>>(f->d_A0, f->d_Qp, d_rho, n1, n1p, p.N);
    ROM_HIP(hipGetLastError());
    ROM_HIP(hipStreamSynchronize(ctx->stream));
  }
  ROM_TRY(dev_alloc(f->tables, &f->d_G, size_t(p.gtotal)));
  for (const FemPlan::GemmG& g : p.gemm_G) {
    TempTables tmp;
    double* d_B = nullptr;
    ROM_TRY(upload(ctx->stream, tmp.list, &d_B, g.Bh));
    ROM_TRY(rom_launch_gemm_nt(ctx, int64_t(hrows), g.rp, n1p, 1.0, f->d_A0, n1p, d_B, n1p, 0.0, f->d_G + g.off, g.rp,
                               "setup_gemm_G"));
    if (!g.entry.empty() && hrows > 0) {  // the entries the distance thresholds declare droppable become exact zeros
      ExtThresholds th;
      memcpy(th.thr, g.thr, sizeof(th.thr));
      k_mask_table<<<unsigned((hrows * g.rp + 255) / 256), 256, 0, ctx->stream>>>(f->d_G + g.off, g.rp, n1, th);
      ROM_HIP(hipGetLastError());
    }
    ROM_HIP(hipStreamSynchronize(ctx->stream));
  }
  ROM_TRY(dev_alloc(f->tables, &f->d_Gs, size_t(p.gstotal)));
  f->gs_bytes = size_t(p.gstotal) * sizeof(double);
  for (const FemPlan::Repack& r : p.repacks) {
    const size_t total = size_t(r.nseg) * hrows * 8;
    if (total == 0) continue;
    k_repack_table<<<unsigned((total + 255) / 256), 256, 0, ctx->stream>>>(f->d_G + r.goff, r.ld, r.nseg, n1, r.orient,
                                                                            f->d_Gs + r.gsoff);
    ROM_HIP(hipGetLastError());
  }
  ROM_HIP(hipStreamSynchronize(ctx->stream));
  return ROM_OK;
}

}  // namespace

extern "C" int rom_fem_destroy(rom_fem* f) {
  if (!f) return ROM_OK;
  hipStreamSynchronize(f->ctx->stream);
  for (void* p : f->tables) hipFree(p);
  // the buffers created on first use
  void* lazy[] = {f->d_L, f->d_invL, f->d_y, f->d_yhat, f->d_dots, f->d_riesz, f->d_green};
  for (void* p : lazy)
    if (p) hipFree(p);
  rom_factored_map_free(f->fmap);
  delete f;
  return ROM_OK;
}

extern "C" int rom_fem_create(rom_ctx* ctx, int nrb, int ncb, int N, rom_fem** out) {
  ROM_CHECK(ctx && out, "rom_fem_create: null argument");
  ROM_CHECK(nrb >= 1 && ncb >= 1 && N >= 2, "rom_fem_create: need nrb,ncb >= 1 and N >= 2 (got %d,%d,%d)", nrb, ncb, N);
  ROM_CHECK(nrb * ncb <= 64, "rom_fem_create: at most 64 blocks supported (got %d)", nrb * ncb);
  ROM_HIP(hipSetDevice(ctx->device));
  FemSwitches sw;
  sw.no_preelim = getenv("ROMHC_NO_PREELIM") != nullptr;
  sw.no_compress = getenv("ROMHC_NO_COMPRESS") != nullptr;
  sw.no_lowrank_ext = getenv("ROMHC_NO_LOWRANK_EXT") != nullptr;
  sw.no_ext_lr = ab_env("ROMHC_NO_EXT_LR") != nullptr;
  sw.verbose = getenv("ROMHC_VERBOSE") != nullptr;
  sw.compress_tol = 1e-14L;
  if (const char* s = getenv("ROMHC_COMPRESS_TOL")) sw.compress_tol = (long double)atof(s);
  sw.no_ext_trunc = getenv("ROMHC_NO_EXT_TRUNC") != nullptr;
  FemPlan p;
  std::string why;
  if (rom_fem_plan(nrb, ncb, N, sw, &p, &why) != ROM_OK) {  // (nothing is allocated yet)
    rom_set_error("%s", why.c_str());
    return ROM_ERR_INVALID;
  }
  // from here on every exit goes through rom_fem_destroy, which frees what has been uploaded so far
  std::unique_ptr<rom_fem, int (*)(rom_fem*)> guard(new rom_fem(), rom_fem_destroy);
  rom_fem* f = guard.get();
  f->ctx = ctx;
  f->nrb = nrb; f->ncb = ncb; f->N = N; f->n1 = p.n1; f->n1p = p.n1p; f->nr = p.nr; f->nc = p.nc; f->dim = p.dim;
  f->nG = p.nG; f->nGp = p.nGp; f->nGa = p.nGa; f->nred = p.nred; f->ncross = p.ncross; f->xb0 = p.xb0; f->T = p.T;
  f->nslots = p.nslots; f->npre = int(p.pre_edges.size()); f->nexp = int(p.exps.size()); f->nrhs = int(p.rhs_terms.size());
  f->spos0 = p.spos0; f->nsc = p.nsc; f->n_all_edges = p.n_all_edges; f->npairs = p.npairs; f->fused1 = p.fused1;
  for (int i = 0; i < 5; ++i) f->wp0[i] = p.wp0[i];
  f->ncoef = p.ncoef; f->ncf = p.ncf; f->nctask = p.nctask; f->ndg = p.ndg; f->ndi = p.ndi; f->n_edges = p.n_edges;
  f->n_lr_blocks = int(p.lr_blocks.size()); f->n_gen_blocks = int(p.gen_blocks.size()); f->lr_nch = p.lr_nch;
  f->nscat = int(p.scat.size()); f->ext_flops = p.ext_flops; f->flops_solve = p.flops_solve; f->bytes_solve = p.bytes_solve;
  f->desc = p.desc; f->slot_of = p.slot_of; f->kptr = p.kptr; f->kpair = p.kpair; f->colptr = p.colptr; f->colrow = p.colrow;
  f->colti = p.colti; f->diag_slot = p.diag_slot; f->sides = p.sides; f->ranks = p.ranks;
#define ROM_UPLOAD(member, vec) ROM_TRY(upload(ctx->stream, f->tables, &f->member, p.vec))
  ROM_UPLOAD(d_pool, pool);         ROM_UPLOAD(d_terms, terms);           ROM_UPLOAD(d_desc, desc);
  ROM_UPLOAD(d_alist, alist);       ROM_UPLOAD(d_aoff, aoff);             ROM_UPLOAD(d_pairs, pairs);
  ROM_UPLOAD(d_pool_acc, pool_acc); ROM_UPLOAD(d_wmeta, wmeta);           ROM_UPLOAD(d_s1_items, s1_items);
  ROM_UPLOAD(d_s1_citems, s1_citems); ROM_UPLOAD(d_dgroups, dgroups);     ROM_UPLOAD(d_dweight, dweight);
  ROM_UPLOAD(d_ditem_group, ditem_group); ROM_UPLOAD(d_ditem_k, ditem_k); ROM_UPLOAD(d_dmat, dmat);
  ROM_UPLOAD(d_P, Ptab);            ROM_UPLOAD(d_Bt, Bt);                 ROM_UPLOAD(d_Qp, Qp);
  ROM_UPLOAD(d_kmax, kmax);         ROM_UPLOAD(d_W, Wz);                  ROM_UPLOAD(d_g, g_red);
  ROM_UPLOAD(d_vec, vecs);          ROM_UPLOAD(d_rhs, rhs_terms);         ROM_UPLOAD(d_pre, pre_edges);
  ROM_UPLOAD(d_exp, exps);          ROM_UPLOAD(d_groups, groups);         ROM_UPLOAD(d_cm, cm);
  ROM_UPLOAD(d_item_group, item_group); ROM_UPLOAD(d_item_k, item_k);     ROM_UPLOAD(d_item_cf, item_cf);
  ROM_UPLOAD(d_ctask, ctask);       ROM_UPLOAD(d_xred, xred);             ROM_UPLOAD(d_scb, scb);
  ROM_UPLOAD(d_kptr, kptr);         ROM_UPLOAD(d_kpair, kpair);           ROM_UPLOAD(d_colptr, colptr);
  ROM_UPLOAD(d_colrow, colrow);     ROM_UPLOAD(d_colti, colti);           ROM_UPLOAD(d_sides, sides);
  ROM_UPLOAD(d_vmap, vmap);         ROM_UPLOAD(d_scat, scat);             ROM_UPLOAD(d_lr_blocks, lr_blocks);
  ROM_UPLOAD(d_gen_blocks, gen_blocks); ROM_UPLOAD(d_epos, epos);         ROM_UPLOAD(d_x128_row, x128_row);
  ROM_UPLOAD(d_x128_flat, x128_flat);
#undef ROM_UPLOAD
  ROM_TRY(build_extension_tables(f, p));
  if (f->fused1)  // (the attribute belongs to the kernel as loaded on this device; setting it again is harmless)
    ROM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_solve1), hipFuncAttributeMaxDynamicSharedMemorySize, S1_LDS_BYTES));
  f->sw_no_fused = getenv("ROMHC_NO_FUSED") != nullptr;
  f->sw_no_ext128 = getenv("ROMHC_NO_EXT128") != nullptr;
  f->sw_no_ext_wave_skip = getenv("ROMHC_NO_EXT_WAVE_SKIP") != nullptr;
#ifdef ROMHC_AB
  // The A/B build (libromhc_ab.so, `make ab`; only tests/ab_variants.py loads it) can FORCE choices that the product makes by
  // geometry -- tilings, workgroup orders, one system per workgroup, tiles assembled in registers -- to check that the forms
  // the product uses on different geometries give the same bits on one.  The product build does not read these.
  // k_extend128's workgroup order: system group fastest once the extension tables outgrow what the caches keep next to
  // the store stream (measured: C5, 4 x 4 / N = 256, tables 100+ MB: fetch 21.7 -> 10.6 GB per launch of 2048 systems, kernel -2...-6 %;
  // C4, 3 x 3 / N = 171: no gain; C2, 16 MB of tables: 5 % slower) -- ROMHC_X128_SYS_FAST = 0 / 1 / 2 overrides
  f->sw_x128_sys_fast = ab_env("ROMHC_X128_SYS_FAST") ? atoi(ab_env("ROMHC_X128_SYS_FAST")) : -1;
  f->sw_no_fold = ab_env("ROMHC_NO_FOLD_EXPAND") != nullptr;
  f->sw_coef_global = ab_env("ROMHC_COEF_GLOBAL") != nullptr;
  f->sw_no_tile_pairs = ab_env("ROMHC_NO_TILE_PAIRS") != nullptr;
  f->sw_no_tile_stream = ab_env("ROMHC_NO_TILE_STREAM") != nullptr;
  f->sw_ext_flat = ab_env("ROMHC_EXT_FLAT") ? (atoi(ab_env("ROMHC_EXT_FLAT")) != 0 ? 1 : 0) : -1;
#endif
  *out = guard.release();
  return ROM_OK;
}
