// Compiled C++ check of BeamSearchOptions::xl (include/fl_compat/flashlight.h) that needs no device: the member exists, defaults
// to false, and CTCLoss::beamSearch (ASGLoss::beamSearch is the same function under its transitions) refuses `xl && wide` with
// std::invalid_argument before it looks at the input (the arrays here are empty: nothing is allocated).  Built with plain g++
// against libw2l_hip.so and run by tests/test_beam_xl_host.py.
#include <iostream>
#include <stdexcept>
#include <string>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

template <class Crit>
static int refuses_both(Crit& crit, const char* name) {
  BeamSearchOptions o;
  o.xl = true;
  o.wide = true;
  try {
    crit.beamSearch(af::array(), af::array(), o);
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("wide and xl") != std::string::npos) return 0;
    std::cerr << name << ": refused, but not for xl && wide: " << e.what() << "\n";
    return 1;
  } catch (const std::exception& e) {
    std::cerr << name << ": not std::invalid_argument: " << e.what() << "\n";
    return 1;
  }
  std::cerr << name << ": xl && wide was accepted\n";
  return 1;
}

int main() {
  BeamSearchOptions o;
  if (o.xl != false || o.wide != false) { std::cerr << "defaults\n"; return 1; }
  int bad = 0;
  {
    CTCLoss crit;
    bad += refuses_both(crit, "CTCLoss");
    // xl alone passes that check: the empty input is what is refused then
    BeamSearchOptions x;
    x.xl = true;
    try {
      crit.beamSearch(af::array(), af::array(), x);
      ++bad;
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("wide and xl") != std::string::npos) ++bad;
    }
  }
  if (bad) return 1;
  std::cout << "beam xl options ok" << std::endl;
  return 0;
}
