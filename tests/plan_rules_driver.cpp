// plan_rules_driver.cpp -- the device-free planner (csrc/plan_rules.hpp) without a device: reads "device LDS_BYTES COMPUTE_UNITS ARCH"
// and one request per line (entry width height upscale precision flags ring out_width out_height align origin_x origin_y span_x
// span_y [sharpen]; floats in hex) from standard input, runs plan_check + plan_geometry on each and prints every PlanGeometry field
// (plan_geometry_print.hpp), or "error CODE TEXT".  A fftup_jit::choose that succeeds stands for a specialisation that loaded.
// Linked with the library's object files (tests/test_host_plan_rules.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "plan_rules.hpp"
#include "plan_geometry_print.hpp"

static int run(const PlanRequest& rq, const DeviceFacts& dev, PlanGeometry& G)
{
    if (int rc = plan_check(rq, G)) return rc;
    if (int rc = plan_geometry_columns(G, dev)) return rc;
    int DD = 1;
    const int D = plan_jit_factor(G, &DD);
    fftup_jit::Choice ch;
    const bool loaded = D && fftup_jit::choose((int)G.W, (int)G.H, D, G.half, stage_radices(G.planUW), ch, wisdom_device_key(G, dev), true, DD);
    ch.u8out = (G.cfg.flags & FFTUP_FLAG_FUSE_U8_STORE) != 0;
    return plan_geometry_finish(G, dev, loaded ? &ch : nullptr);
}

int main()
{
    DeviceFacts dev;
    std::string line, word;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> word;
        if (word == "device") { in >> dev.lds_bytes >> dev.compute_units >> dev.arch; continue; }
        fftup_config cfg{};
        std::string f[5];
        uint32_t size[2], align;
        in >> cfg.width >> cfg.height >> f[0] >> cfg.precision >> cfg.flags >> cfg.ring >> size[0] >> size[1] >> align >> f[1] >> f[2] >> f[3] >> f[4];
        if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
        cfg.channels = 3; cfg.sharpen = 0.2f; cfg.upscale = strtof(f[0].c_str(), nullptr);
        if (std::string s; in >> s) cfg.sharpen = strtof(s.c_str(), nullptr);          // (optional last field: the strength, 0.2 without it)
        const fftup_view view = {strtod(f[1].c_str(), nullptr), strtod(f[2].c_str(), nullptr), strtod(f[3].c_str(), nullptr), strtod(f[4].c_str(), nullptr)};
        PlanRequest rq;
        rq.cfg = &cfg;
        if (word != "create") { rq.size = size; rq.align = align; }
        if (word == "view") rq.view = &view;
        PlanGeometry G;
        if (int rc = run(rq, dev, G)) { printf("error %d %s\n", rc, fftup_last_error()); continue; }
        print_geometry(stdout, G, G.bzL, G.viewL);
    }
    return 0;
}
