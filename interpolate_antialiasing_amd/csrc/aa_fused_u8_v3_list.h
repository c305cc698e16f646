// aa_fused_u8_v3_list.h — the compiled set of the fused uint8 kernel (aa_fused_u8_v3_impl.h), written once.  An X-macro list, included
// repeatedly: the includer defines V3_ROUTE and / or V3_UNIT first.
//
// V3_ROUTE(route, TW with Pillow arithmetic, TW with float arithmetic, MAXC, forms): a route's window widths, open-output-row counts and
// forms.  A form is a set of V3Forms bits: T = TWO_DMA (wide segments, generic window addressing), N = NONNEG, P = PERIODIC, U2 / U6 =
// UPK 2 / 6.  Float arithmetic has no NONNEG or PERIODIC form: its kernels are the forms with those two bits cleared.  A route compiles
// TW x MAXC x forms; PL (plane groups), SP (split windows) and ALPHA follow from the route.
//
// V3_UNIT(name, route, C, arithmetic, fast): one translation unit, aa_fused_u8_v3_unit.hip compiled into aa_fused_u8_v3_<name>.o with
// -DAA_V3_UNIT=<name> (and -DAA_V3_FLT_FAST=1 when fast is 1: the tolerance mode, AA_FLAG_FAST).  The Makefile reads the names and the
// fast column from these rows: keep one row per line.  C is the kernel's template C (3 for plane groups of single-channel planes);
// arithmetic is PIL, FLT or BOTH.  The units split the set so that it compiles in parallel.

#ifndef V3_ROUTE
#define V3_ROUTE(...)
#endif
#ifndef V3_UNIT
#define V3_UNIT(...)
#endif

//       route      TW, Pillow            TW, float       MAXC          forms
V3_ROUTE(NARROW,    (2, 4, 6, 8, 12, 16), (6, 8, 12, 16), (2, 3, 4),    (T | N, T, N | P, N, P, 0))
V3_ROUTE(WIDE,      (24, 34),             (24, 34),       (2, 3, 4, 6), (T | N, T, N, 0))  // 17 .. 34 taps
V3_ROUTE(SPLIT,     (16, 24, 34),         (),             (2, 3, 4, 6), (T | N, T, N, 0))  // 35 .. 136 taps, TW per lane
V3_ROUTE(SIX,       (6, 8, 12, 16),       (6, 8, 12, 16), (6),          (0))               // 5-6 open rows, Hamming / Lanczos
V3_ROUTE(UP,        (2, 4, 6, 8, 12, 16), (6, 8, 12, 16), (1),          (N | U2, U6))      // growing heights
V3_ROUTE(PLANES,    (4, 6, 8, 12),        (6, 8),         (2, 3, 4),    (N, 0))            // three planes per wave
V3_ROUTE(ALPHA,     (2, 4, 6, 8, 12, 16), (),             (2, 4),       (N, 0))            // straight alpha
V3_ROUTE(SIX_ALPHA, (6, 8, 12, 16),       (),             (6),          (0))               // ... with 5-6 open rows

//      name   route      C  arithmetic fast
V3_UNIT(c1,    NARROW,    1, PIL,       0)
V3_UNIT(c3,    NARROW,    3, PIL,       0)
V3_UNIT(c4,    NARROW,    4, PIL,       0)
V3_UNIT(c1f,   NARROW,    1, FLT,       0)
V3_UNIT(c3f,   NARROW,    3, FLT,       0)
V3_UNIT(c4f,   NARROW,    4, FLT,       0)
V3_UNIT(c1ff,  NARROW,    1, FLT,       1)
V3_UNIT(c3ff,  NARROW,    3, FLT,       1)
V3_UNIT(c4ff,  NARROW,    4, FLT,       1)
V3_UNIT(c1w,   WIDE,      1, PIL,       0)
V3_UNIT(c3w,   WIDE,      3, PIL,       0)
V3_UNIT(c4w,   WIDE,      4, PIL,       0)
V3_UNIT(c1s,   SPLIT,     1, PIL,       0)
V3_UNIT(c3s,   SPLIT,     3, PIL,       0)
V3_UNIT(c4s,   SPLIT,     4, PIL,       0)
V3_UNIT(c1wf,  WIDE,      1, FLT,       0)
V3_UNIT(c3wf,  WIDE,      3, FLT,       0)
V3_UNIT(c4wf,  WIDE,      4, FLT,       0)
V3_UNIT(c3g,   PLANES,    3, PIL,       0)
V3_UNIT(c3gf,  PLANES,    3, FLT,       0)
V3_UNIT(c3gff, PLANES,    3, FLT,       1)
V3_UNIT(c1u,   UP,        1, BOTH,      0)
V3_UNIT(c3u,   UP,        3, BOTH,      0)
V3_UNIT(c4u,   UP,        4, BOTH,      0)
V3_UNIT(c1l,   SIX,       1, PIL,       0)
V3_UNIT(c3l,   SIX,       3, PIL,       0)
V3_UNIT(c4l,   SIX,       4, PIL,       0)
V3_UNIT(c1lf,  SIX,       1, FLT,       0)
V3_UNIT(c3lf,  SIX,       3, FLT,       0)
V3_UNIT(c4lf,  SIX,       4, FLT,       0)
V3_UNIT(c4a,   ALPHA,     4, PIL,       0)
V3_UNIT(c4al,  SIX_ALPHA, 4, PIL,       0)

#undef V3_ROUTE
#undef V3_UNIT
