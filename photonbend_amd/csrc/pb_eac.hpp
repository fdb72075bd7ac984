// pb_eac.hpp - the two functions that make a cube map equi-angular (PB_KIND_EAC).  An equi-angular cube is the plain
// cube in everything but the scale along each face axis: a centred face coordinate c (pixels from the face centre,
// half = N / 2) is proportional to the ANGLE from the face centre instead of its tangent.
//   warp    EAC face coordinate -> gnomonic (plain cube) face coordinate   np.tan((c / half) * Q) * half
//   unwarp  and back                                                        (np.arctan(c / half) * IQ) * half
// Q = pi / 4 and IQ = 4 / pi as float64; every operation rounded on its own in exactly this nesting (-ffp-contract=off), np.tan and
// np.arctan the functions pb_math.hpp restates bit for bit for both math flavours.  Host and device compile this very text
// (tests/c_host/eac_warp_host.cpp is the host's).
#pragma once
#include "pb_math.hpp"

#define PB_EAC_Q 0x1.921fb54442d18p-1   // math.pi / 4
#define PB_EAC_IQ 0x1.45f306dc9c883p+0  // 4 / math.pi

PB_MATH_FN double pb_eac_warp(double c, double half) { return pb_tan_np((c / half) * PB_EAC_Q) * half; }
PB_MATH_FN double pb_eac_unwarp(double c, double half) { return (pb_atan_np(c / half) * PB_EAC_IQ) * half; }
