// Compiled C++ check of BeamSearchOptions::manyTokens (include/fl_compat/flashlight.h) that needs no device: the member exists,
// defaults to false, CTCLoss::beamSearch (ASGLoss::beamSearch is the same function under its transitions) refuses it together
// with `wide`, with `xl` and with `lmToken` with std::invalid_argument before it looks at the input (the arrays here are empty:
// nothing is allocated), and alone it passes those checks (the empty input is what is refused then).  Built with plain g++ against
// libw2l_hip.so and run by tests/test_beam_mt_host.py.
#include <iostream>
#include <stdexcept>
#include <string>

#include "fl_compat/flashlight.h"

using namespace fl;
using namespace fl::pkg::speech;

// 0: refused with std::invalid_argument whose text holds `what`; 1 otherwise
static int refuses(CTCLoss& crit, const BeamSearchOptions& o, const char* what, const char* name) {
  try {
    crit.beamSearch(af::array(), af::array(), o);
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find(what) != std::string::npos) return 0;
    std::cerr << name << ": refused, but not for the conflict: " << e.what() << "\n";
    return 1;
  } catch (const std::exception& e) {
    std::cerr << name << ": not std::invalid_argument: " << e.what() << "\n";
    return 1;
  }
  std::cerr << name << ": accepted\n";
  return 1;
}

int main() {
  BeamSearchOptions d;
  if (d.manyTokens != false || d.xl != false || d.wide != false || d.lmToken != false) { std::cerr << "defaults\n"; return 1; }
  int bad = 0;
  CTCLoss crit;
  { BeamSearchOptions o; o.manyTokens = true; o.wide = true; bad += refuses(crit, o, "manyTokens is a kernel family of its own", "wide"); }
  { BeamSearchOptions o; o.manyTokens = true; o.xl = true; bad += refuses(crit, o, "manyTokens is a kernel family of its own", "xl"); }
  { BeamSearchOptions o; o.manyTokens = true; o.lmToken = true; bad += refuses(crit, o, "lmToken has no many-token family", "lmToken"); }
  {   // alone it passes: the empty input is what is refused
    BeamSearchOptions o;
    o.manyTokens = true;
    o.beamSize = 8192;
    o.beamSizeToken = 256;
    bad += refuses(crit, o, "bad input or options", "alone");
  }
  {   // the beam sessions keep 64 tokens per frame
    BeamSearchOptions o;
    o.manyTokens = true;
    try {
      StreamingDecoder dec(1, 8, 64, 30, o);
      std::cerr << "StreamingDecoder accepted manyTokens\n";
      ++bad;
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("manyTokens") == std::string::npos) { std::cerr << "StreamingDecoder: " << e.what() << "\n"; ++bad; }
    } catch (const std::exception& e) {
      std::cerr << "StreamingDecoder: not std::invalid_argument: " << e.what() << "\n";
      ++bad;
    }
  }
  if (bad) return 1;
  std::cout << "beam mt options ok" << std::endl;
  return 0;
}
