// aa_fused_float_list.h — the compiled set of the fused float kernels, written once.  An X-macro list, included repeatedly: the includer
// defines F32_SET and / or F32_UNIT first.
//
// F32_SET(unit, element types, CS, widths): kernels of one unit.  Shrinking heights (fused_f32_nchw_kernel): CS is the channel stride
// (1: planes, 3 / 4: fp32 / fp16 / bf16 channels_last), the widths are NQ.  Growing heights (fused_f32_nchw_up_kernel): CS is CPL, the widths are U;
// CPL * U lane masks fit the scalar registers (<= 20).  The plan takes the smallest width that holds the window.
//
// F32_UNIT(name, kernel, fast, MAXC or KR, G, NDMA): one translation unit, aa_fused_float_unit.hip compiled into aa_fused_float_<name>.o with
// -DAA_F32_UNIT=<name> (and -DAA_F32_FAST=1 when fast is 1: the tolerance mode).  The Makefile reads these rows: keep one per line.  A unit
// compiles each of its kernels with every MAXC or KR and every staging form: G rows per wave, NDMA DMAs of 64 16-byte pieces per row (the
// two lists pair up).  The plan takes the smallest MAXC / KR that holds the H table's rows and the smallest NDMA that holds the segment.

#ifndef F32_SET
#define F32_SET(...)
#endif
#ifndef F32_UNIT
#define F32_UNIT(...)
#endif

//      unit  element types           CS  NQ
F32_SET(down, (AA_F32, AA_F16, AA_BF16), 1, (2, 3, 4, 5, 7, 9, 11))  // (9: 33 taps, bicubic 906 -> 120 thumbnails; 11: 41, 4K -> 224 bilinear)
F32_SET(down, (AA_F64),                  1, (2, 4, 6, 8, 11))
F32_SET(down, (AA_F32),                  3, (2, 3, 4, 5, 7, 9))
F32_SET(down, (AA_F32),                  4, (2, 3, 4, 5, 7, 9))
F32_SET(nhwc16, (AA_F16, AA_BF16),       3, (2, 3, 4, 5, 7, 9))  // (a unit of its own: in `down` they would add 63 % to its kernels)
F32_SET(nhwc16, (AA_F16, AA_BF16),       4, (2, 3, 4, 5, 7, 9))
F32_SET(fast, (AA_F32, AA_F16, AA_BF16), 1, (2, 3, 4, 5, 7, 9, 11))  // (what it lacks, the tolerance mode runs exact)
//      unit  element types           CPL U
F32_SET(up,   (AA_F32, AA_F16, AA_BF16), 4, (2, 3, 4, 5))
F32_SET(up,   (AA_F32, AA_F16, AA_BF16), 2, (2, 3, 4, 5, 6, 8))
F32_SET(up,   (AA_F32, AA_F16, AA_BF16), 1, (2, 3, 4, 5, 6, 8))

// G 4 for two DMAs per row: rings stay <= 8 KiB per wave.  G 8 there measured the same within noise on config 2 (exact 0.192 | 0.193 ms,
// tolerance mode 0.162-0.176 | 0.166-0.180): the deeper ring buys nothing.  The gather kernel stages one DMA per row.
//       name  kernel fast MAXC / KR     G       NDMA
F32_UNIT(down, DOWN,  0,   (2, 3, 4, 6), (8, 4), (1, 2))
F32_UNIT(fast, DOWN,  1,   (2, 3, 4, 6), (8, 4), (1, 2))
F32_UNIT(nhwc16, DOWN, 0,  (2, 3, 4, 6), (8, 4), (1, 2))
F32_UNIT(up,   UP,    0,   (2, 4, 6),    (8),    (1))

#undef F32_SET
#undef F32_UNIT
