# decode_lextok_caller, the compiled caller of beamSearch with a token LM under a lexicon (tests/test_gpu_beam_lextok_surfaces.py), built by the rules of the
# Makefile beside it -- its compiler, flags and libraries -- through a target of its own:
#   make -C tests/cpp -f decode_lextok_caller.mk decode_lextok_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/decode_lextok_caller: decode_lextok_caller.cpp ../../include/fl_compat/flashlight.h ../../include/fl_compat/lexicon.h ../../include/fl_compat/lm.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: decode_lextok_caller
decode_lextok_caller: $(OUT)/decode_lextok_caller
