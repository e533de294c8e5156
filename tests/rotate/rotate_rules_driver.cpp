// rotate_rules_driver.cpp -- the rotator's device-free rules (csrc/plan_rules.hpp, rotate_geometry) without a device: reads one
// request per line (width height precision max_batch) from standard input and prints "ok max_batch TK lds_x lds_y" or
// "error CODE TEXT".  Linked with the library's object files (tests/test_host_rotate.py), in the manner of
// tests/align_rules_driver.cpp.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "plan_rules.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        fftup_rotate_config c{};
        in >> c.width >> c.height >> c.precision >> c.max_batch;
        if (!in) { fprintf(stderr, "bad request line: %s\n", line.c_str()); return 2; }
        RotateGeometry G;
        if (int rc = rotate_geometry(c, G)) { printf("error %d %s\n", rc, fftup_last_error()); continue; }
        printf("ok %u %u %zu %zu\n", G.max_batch, G.TK, G.lds_x, G.lds_y);
    }
    return 0;
}
