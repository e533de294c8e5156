// roll_rules_driver.cpp -- the roll estimator's device-free rules (csrc/plan_rules.hpp, roll_geometry) without a device: reads one
// request per line (width height precision window_w window_h decimate band angles upsample max_batch; band as a hex float) from
// standard input and prints "ok d window_w window_h crop_x crop_y upsample n angles rho_min rho_max m_band K max_batch cx cy" or
// "error CODE TEXT".  tests/test_host_roll.py compiles it TOGETHER with csrc/plan_rules.cpp under the address and
// undefined-behaviour sanitizers (host code only) and links the rest from the library's object files.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "plan_rules.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        fftup_roll_config c{};
        std::string band;
        in >> c.width >> c.height >> c.precision >> c.window_w >> c.window_h >> c.decimate >> band >> c.angles >> c.upsample >> c.max_batch;
        if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
        c.band = strtof(band.c_str(), nullptr);
        RollGeometry G;
        if (int rc = roll_geometry(c, G)) { printf("error %d %s\n", rc, fftup_last_error()); continue; }
        printf("ok %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", G.d, G.nx, G.ny, G.crop_x, G.crop_y, G.kappa, G.n, G.ntheta, G.rho_min, G.rho_max,
               G.mb, G.K, G.max_batch, G.cx, G.cy);
    }
    return 0;
}
