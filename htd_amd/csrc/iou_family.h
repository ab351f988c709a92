// The IoU-family box losses on decoded boxes with their derivatives, in fp64: shared by box_ops.hip (htd_roi_head_loss_decoded)
// and fcos.hip (htd_fcos_loss).
#pragma once
#include "common.h"

namespace {

// ---- IoU-family regression losses on decoded boxes (losses/iou_loss.py:11-209) with their derivatives ---------------------
// Autograd's conventions at the non-differentiable points are kept (tests/golden/iou_loss.npz, tie set): a two-operand
// max / min splits the gradient evenly at a tie, clamp passes it at its bound, |x| has slope 0 at 0.
enum { BOX_IOU = 0, BOX_BOUNDED = 1, BOX_GIOU = 2, BOX_DIOU = 3, BOX_CIOU = 4 };

struct Box { double x1, y1, x2, y2; };

__device__ __forceinline__ double max_tie(double a, double b, double &da)       // max(a, b), da = d/da
{
    da = a > b ? 1. : (a == b ? 0.5 : 0.);
    return fmax(a, b);
}

__device__ __forceinline__ double min_tie(double a, double b, double &da)
{
    da = a < b ? 1. : (a == b ? 0.5 : 0.);
    return fmin(a, b);
}

// loss of kinds iou / giou / diou / ciou for prediction p against target t, G = d loss / d p
__device__ __forceinline__ double iou_family_loss(int kind, Box p, Box t, double eps, Box &G)
{
    // intersection, areas
    double dltx, dlty, drbx, drby;
    const double ltx = max_tie(p.x1, t.x1, dltx), lty = max_tie(p.y1, t.y1, dlty);
    const double rbx = min_tie(p.x2, t.x2, drbx), rby = min_tie(p.y2, t.y2, drby);
    const double iw0 = rbx - ltx, ih0 = rby - lty;
    const double iw = fmax(iw0, 0.), ih = fmax(ih0, 0.);
    const double giw = iw0 >= 0. ? 1. : 0., gih = ih0 >= 0. ? 1. : 0.;
    const double ov = iw * ih;
    const Box dov = {-ih * giw * dltx, -iw * gih * dlty, ih * giw * drbx, iw * gih * drby};
    const double pw = p.x2 - p.x1, ph = p.y2 - p.y1;
    const double ap = pw * ph, ag = (t.x2 - t.x1) * (t.y2 - t.y1);
    const double un0 = ap + ag - ov;
    double un, gu;
    if (kind == BOX_IOU || kind == BOX_GIOU) { un = max_tie(un0, eps, gu); }        // bbox_overlaps: max(union, eps)
    else { un = un0 + eps; gu = 1.; }                                              // diou / ciou: union + eps
    const Box dun = {gu * (-ph - dov.x1), gu * (-pw - dov.y1), gu * (ph - dov.x2), gu * (pw - dov.y2)};
    const double iou = ov / un;
    const Box diou = {(dov.x1 - iou * dun.x1) / un, (dov.y1 - iou * dun.y1) / un, (dov.x2 - iou * dun.x2) / un,
                      (dov.y2 - iou * dun.y2) / un};
    if (kind == BOX_IOU) {      // the reference's edit: clamp(min=eps), IoUs of at most 0.1 lifted by 0.1, -log
        const double c = fmax(iou, eps);
        const double v = c > 0.1 ? c : 0.1 + c;
        const double s = iou >= eps ? -1. / v : 0.;
        G = {s * diou.x1, s * diou.y1, s * diou.x2, s * diou.y2};
        return -log(v);
    }
    // enclosing box
    double dex1, dey1, dex2, dey2;
    const double ex1 = min_tie(p.x1, t.x1, dex1), ey1 = min_tie(p.y1, t.y1, dey1);
    const double ex2 = max_tie(p.x2, t.x2, dex2), ey2 = max_tie(p.y2, t.y2, dey2);
    const double ew0 = ex2 - ex1, eh0 = ey2 - ey1;
    const double ew = fmax(ew0, 0.), eh = fmax(eh0, 0.);
    const double gew = ew0 >= 0. ? 1. : 0., geh = eh0 >= 0. ? 1. : 0.;
    if (kind == BOX_GIOU) {
        double gea;
        const double ea = max_tie(ew * eh, eps, gea);
        const Box dea = {-gea * eh * gew * dex1, -gea * ew * geh * dey1, gea * eh * gew * dex2, gea * ew * geh * dey2};
        const double hole = (ea - un) / ea;                       // d hole = (dea - dun) / ea - hole * dea / ea
        G = {-(diou.x1 - ((dea.x1 - dun.x1) - hole * dea.x1) / ea), -(diou.y1 - ((dea.y1 - dun.y1) - hole * dea.y1) / ea),
             -(diou.x2 - ((dea.x2 - dun.x2) - hole * dea.x2) / ea), -(diou.y2 - ((dea.y2 - dun.y2) - hole * dea.y2) / ea)};
        return 1. - (iou - hole);
    }
    // squared centre distance over the squared diagonal of the enclosing box
    const double c2 = ew * ew + eh * eh + eps;
    const Box dc2 = {-2. * ew * gew * dex1, -2. * eh * geh * dey1, 2. * ew * gew * dex2, 2. * eh * geh * dey2};
    const double sx = (t.x1 + t.x2) - (p.x1 + p.x2), sy = (t.y1 + t.y2) - (p.y1 + p.y2);
    const double rho2 = sx * sx / 4. + sy * sy / 4.;
    const double q = rho2 / c2;
    const Box dq = {(-0.5 * sx - q * dc2.x1) / c2, (-0.5 * sy - q * dc2.y1) / c2, (-0.5 * sx - q * dc2.x2) / c2,
                    (-0.5 * sy - q * dc2.y2) / c2};
    if (kind == BOX_DIOU) {
        G = {dq.x1 - diou.x1, dq.y1 - diou.y1, dq.x2 - diou.x2, dq.y2 - diou.y2};
        return 1. - (iou - q);
    }
    // ciou: aspect-ratio term v^2 / (1 - iou + v), eps on the heights only
    const double h1 = ph + eps, h2 = (t.y2 - t.y1) + eps;
    const double r1 = pw / h1;
    const double a = atan((t.x2 - t.x1) / h2) - atan(r1);
    const double factor = 0.40528473456935109;                    // 4 / pi^2
    const double v = factor * (a * a);
    const double dvdr = -2. * factor * a / (1. + r1 * r1);      // d v / d r1
    const Box dv = {dvdr * (-1. / h1), dvdr * (r1 / h1), dvdr * (1. / h1), dvdr * (-r1 / h1)};
    // v == 0 makes the term 0 with zero slope, also where 1 - iou + v is 0 (pred == target with a union that swallows eps: the
    // reference's fp32 form yields 0 / 0 there): the limit, as in the tensor formulation (losses.py:ciou_loss)
    double term = 0.;
    Box dterm = {0., 0., 0., 0.};
    if (v != 0.) {
        const double den = 1. - iou + v;
        term = v * v / den;
        const double k1 = 2. * v / den, k2 = term / den;
        dterm = {k1 * dv.x1 - k2 * (dv.x1 - diou.x1), k1 * dv.y1 - k2 * (dv.y1 - diou.y1), k1 * dv.x2 - k2 * (dv.x2 - diou.x2),
                 k1 * dv.y2 - k2 * (dv.y2 - diou.y2)};
    }
    G = {dq.x1 + dterm.x1 - diou.x1, dq.y1 + dterm.y1 - diou.y1, dq.x2 + dterm.x2 - diou.x2, dq.y2 + dterm.y2 - diou.y2};
    return 1. - (iou - (q + term));
}

}  // namespace
