// Host-side launch plumbing shared by every entry point: the 32-bit view binder and the experiment-knob readers.
// Plain C++17, no HIP include: tests/host/launch_host_check.cpp builds it with the host compiler alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/mgdt.h"

// ---- views behind 32-bit buffer descriptors ----
// Bytes from the view's first element to one past its last one (positive strides).
static inline long view_extent_bytes(const mgdt_view* v, int elem_bytes) {
  return ((long)(v->n - 1) * v->sn + (long)(v->h - 1) * v->sh + (long)(v->w - 1) * v->sw + v->c) * elem_bytes;
}

// 32-bit offsets reach every byte of the view (the descriptor's range check does the rest)
static inline bool view_spans_32bit(const mgdt_view* v, int elem_bytes) { return view_extent_bytes(v, elem_bytes) < 0x7fffffffL; }

// sn, sh, sw in multiples of q elements and the pointer in multiples of q * elem_bytes bytes
static inline bool view_aligned(const mgdt_view* v, int q, int elem_bytes) {
  return v->sw % q == 0 && v->sh % q == 0 && v->sn % q == 0 && (uintptr_t)v->p % ((uintptr_t)q * elem_bytes) == 0;
}

// What one call site asks of a view before its kernel may address it through {pointer, int byte strides, uint32 extent}.  Every site states its
// own: the limits follow from that kernel's addressing and are not meant to agree.
struct ViewPolicy {
  int align;          // sn, sh, sw multiples of `align` elements and the pointer of align * elem_bytes bytes; 0 = not tested
  bool nhwc;          // sc == 1 required
  long row_limit;     // sh * elem_bytes must stay below it (24-bit multiplies: 1 << 23); 0 = not tested
  long pix_limit;     // sw * elem_bytes likewise
  bool skip_null;     // a null view / null pointer is an absent operand: nothing is written, nothing is refused
};

// False = refused (outputs untouched).  The extent must stay below 2^31 - 1 at every site (view_spans_32bit).
static inline bool bind_view(const mgdt_view* v, int elem_bytes, const ViewPolicy& pol, const char** p, int* sn, int* sh, int* sw, uint32_t* bytes) {
  if (!v || !v->p) return pol.skip_null;
  const long sz = elem_bytes;
  if (pol.nhwc && v->sc != 1) return false;
  if (pol.align && !view_aligned(v, pol.align, elem_bytes)) return false;
  if (!view_spans_32bit(v, elem_bytes)) return false;
  if (pol.row_limit && v->sh * sz >= pol.row_limit) return false;
  if (pol.pix_limit && v->sw * sz >= pol.pix_limit) return false;
  *p = (const char*)v->p; *sn = (int)(v->sn * sz); *sh = (int)(v->sh * sz); *sw = (int)(v->sw * sz); *bytes = (uint32_t)view_extent_bytes(v, elem_bytes);
  return true;
}

// The same tests for a site that keeps its own (64-bit) strides.
static inline bool view_fits(const mgdt_view* v, int elem_bytes, const ViewPolicy& pol) {
  const char* p; int sn, sh, sw; uint32_t bytes;
  return bind_view(v, elem_bytes, pol, &p, &sn, &sh, &sw, &bytes);
}

// ---- experiment knobs (environment; none is part of the ABI) ----
// knob_*: read the environment now; a call site that uses them bare follows the variable from call to call (the tests flip those at run time).
// KNOB_ONCE(knob_*(...)): the first value that this call site (each instantiation of a template apart) sees holds for the life of the process.
// Garbage parses as atoi / atol parse it ("x" = 0, "07" = 7, "" = 0); a pair that does not scan as "a,b" reads as unset.
static inline bool knob_set(const char* name) { return getenv(name) != nullptr; }
static inline int knob_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline long knob_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
static inline bool knob_unless0(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }     // off only by a value that starts with '0'
static inline bool knob_pair(const char* name, int* a, int* b) {
  const char* e = getenv(name);
  int x = 0, y = 0;
  if (!e || sscanf(e, "%d,%d", &x, &y) != 2) return false;
  *a = x; *b = y;
  return true;
}
#define KNOB_ONCE(read) ([] { static const auto once_ = (read); return once_; }())

static inline int knob_stem_wgs() { return knob_int("MGDT_STEM_WGS", 0); }     // stem2_geometry and the launch must agree on the grid

/* Every knob.  "call" = read on every call, "once" = KNOB_ONCE; "set" = any value, the empty one included.
 * knob                      values                                                                           read  file
 * MGDT_BN_V                 int, 4; 8 = 16-byte bf16 vectors in the batch-norm kernels                       once  bn_fast.hip
 * MGDT_C3_DBG               set = phase stamps of every workgroup on stderr                                  call  conv3x3_lds.hip
 * MGDT_C3_WAVES8            int, 1; 0 = the four-wave form everywhere                                        once  conv3x3_lds.hip
 * MGDT_CNX_DBG              set = phase stamps                                                               call  cnx_block.hip
 * MGDT_CONV3_LDS            int, 1; 0 = never the LDS-staged 3x3 kernel, 2 / 3 = also its slower forms       once  conv3x3_lds.hip
 * MGDT_CONV_GCAP            int, 256 (8 waves) / 1024; cap on the persistent grid                            call  conv_igemm.hip
 * MGDT_CONV_MINWG           int, 128; fewer workgroups than this split the couts                             call  conv_igemm.hip
 * MGDT_CONV_MT1             int; 4 = MT 4 on one-cout-block layers                                           call  conv_igemm.hip
 * MGDT_CONV_PANEL_KIB       int, 144; weight panel cap in KiB                                                call  conv_igemm.hip
 * MGDT_CONV_TAIL_SPLIT      set = halve NT for 769..960 workgroups                                           once  conv_igemm.hip
 * MGDT_CONV_WAVES           int, 8; clamped to 1..8 waves per workgroup                                      call  conv_igemm.hip
 * MGDT_CSP_COMPACT          on unless the value starts with '0' = the linear pixel walk                      call  csp_block.hip
 * MGDT_CSP_DBG              set = phase stamps                                                               call  csp_block.hip
 * MGDT_CSP_PAIR             on unless the value starts with '0' = the unpaired wd = 8 form                   call  csp_block.hip
 * MGDT_CSP_TILE             "th,tw" = force the tile                                                         call  csp_block.hip, csp_c3.hip
 * MGDT_DW_DBG               set = phase stamps                                                               call  pointwise.hip
 * MGDT_DW_TS                int, 0; 8 / 10 = pick the row kernel of dwconv7_ln                               once  pointwise.hip
 * MGDT_MLP_DBG              set = phase stamps                                                               call  mlp_chain.hip
 * MGDT_NMS_DBG              set = phase clocks                                                               call  nms.hip
 * MGDT_SPPF_CHAINED         set = the chained three-pass SPPF kernel                                         once  pointwise.hip
 * MGDT_SPPF_DBG             set = phase stamps                                                               call  sppf_fused.hip
 * MGDT_SPR_DBG              set = phase stamps                                                               call  pointwise.hip
 * MGDT_SPR_KMAX             long, 12; workgroups per image at most                                           once  pointwise.hip
 * MGDT_SPR_VECS             long, 2048; vectors per workgroup                                                once  pointwise.hip
 * MGDT_STEM_DBG             set = phase sums                                                                 call  stem_fused.hip
 * MGDT_STEM_WGS             int, 0 = no cap; cap on the persistent grid                                      call  stem_fused.hip
 * MGDT_WGRAD_DBG            set = print the wave arrangement                                                 once  wgrad_bf16.hip
 * MGDT_WGRAD_F32MFMA        set = fp32 MFMA for bf16 tensors too                                             once  train.hip
 * MGDT_WGRAD_FILL           long, 448; 0 = off; workgroups to reach with extra splits                        once  train.hip
 * MGDT_WGRAD_PARTIAL_ELEMS  long, 4 Mi; budget of the partial sums in elements                               once  train.hip
 * MGDT_WGRAD_SPLITS         long, 512; cap on the splits                                                     once  train.hip
 * MGDT_WGRAD_VALU           set = the VALU outer-product kernel                                              once  train.hip
 */
