// plan_geometry_print.hpp -- every decision field of a plan (PlanGeometry, csrc/plan_rules.hpp) as one line of name=value
// pairs: what tests/plan_rules_driver.cpp prints and tests/golden/plan_geometry.json records.  Floats as hex, a StagePlan as
// n:r.r.r, a four-step split as on,n1,n2,tka,tkb,p1,p2,ldsA,ldsB,thrA,thrB.
#pragma once
#include <cstdio>
#include <string>

template <class S> static std::string stage_text(const S& p)
{
    std::string s = std::to_string(p.n) + ":";
    for (int i = 0; i < p.nstages; i++) s += (i ? "." : "") + std::to_string((int)p.radix[i]);
    return s;
}

template <class F> static std::string four_text(const F& f)
{
    char t[256];
    snprintf(t, sizeof t, "%d,%d,%d,%d,%d,%s,%s,%zu,%zu,%d,%d", (int)f.on, f.n1, f.n2, f.tka, f.tkb, stage_text(f.p1).c_str(), stage_text(f.p2).c_str(),
             f.ldsA, f.ldsB, f.thrA, f.thrB);
    return t;
}

// bzL: the Bluestein lengths of W, H, uW, uH (0: a direct transform); viewL: the convolution lengths of a view plan's axes
template <class G> static void print_geometry(FILE* f, const G& g, const unsigned bzL[4], const unsigned viewL[2])
{
    fprintf(f, "W=%u H=%u uW=%u uH=%u ring=%u half=%d dbl=%d esz=%zu csz=%zu", g.W, g.H, g.uW, g.uH, g.ring, (int)g.half, (int)g.dbl, g.esz, g.csz);
    fprintf(f, " TK=%d NT=%d ncols=%d zlx=%d zrx=%d zly=%d zry=%d", g.TK, g.NT, g.ncols, g.zlx, g.zrx, g.zly, g.zry);
    fprintf(f, " planW=%s planH=%s planUW=%s planUH=%s", stage_text(g.planW).c_str(), stage_text(g.planH).c_str(), stage_text(g.planUW).c_str(), stage_text(g.planUH).c_str());
    fprintf(f, " thrW=%d thrCol=%d thrUW=%d ldsRowF=%zu ldsCol=%zu ldsRowI=%zu upsq=%a coef=%a", g.thrW, g.thrCol, g.thrUW, g.ldsRowF, g.ldsCol, g.ldsRowI, (double)g.upsq, (double)g.coef);
    fprintf(f, " family=%d tuned=%d fused=%d u8out=%d mixed=%d U=%d cplx=%d dct=%d down=%d poly=%d inplaceC=%d inplaceF=%d inplaceI=%d", (int)g.family, (int)g.tuned,
            (int)g.fused, (int)g.u8out, g.mixed, g.U, (int)g.cplx, (int)g.dct, (int)g.down, (int)g.poly, (int)g.inplaceC, (int)g.inplaceF, (int)g.inplaceI);
    fprintf(f, " fourF=%s fourI=%s colF=%s colI=%s", four_text(g.fourF).c_str(), four_text(g.fourI).c_str(), four_text(g.colF).c_str(), four_text(g.colI).c_str());
    fprintf(f, " bzL=%u,%u,%u,%u bz=%d odd=%d exact=%d align=%u view=%d viewL=%u,%u pairs_per_strip=%d\n", bzL[0], bzL[1], bzL[2], bzL[3], (int)g.bz, (int)g.odd,
            (int)g.exact, g.align, (int)g.view, viewL[0], viewL[1], g.pairs_per_strip);
}
