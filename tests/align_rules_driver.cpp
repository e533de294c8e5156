// align_rules_driver.cpp -- the aligner's device-free rules (csrc/plan_rules.hpp, align_geometry) without a device: reads one
// request per line (width height precision window_w window_h decimate band upsample max_batch; band as a hex float) from standard
// input and prints "ok d window_w window_h crop_x crop_y upsample band_kx band_ky" or "error CODE TEXT".  Linked with the library's
// object files (tests/test_host_align.py), in the manner of tests/plan_rules_driver.cpp.
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
        fftup_align_config c{};
        std::string band;
        in >> c.width >> c.height >> c.precision >> c.window_w >> c.window_h >> c.decimate >> band >> c.upsample >> c.max_batch;
        if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
        c.band = strtof(band.c_str(), nullptr);
        AlignGeometry G;
        if (int rc = align_geometry(c, G)) { printf("error %d %s\n", rc, fftup_last_error()); continue; }
        printf("ok %u %u %u %u %u %u %u %u\n", G.d, G.nx, G.ny, G.crop_x, G.crop_y, G.kappa, G.band_kx, G.band_ky);
    }
    return 0;
}
