# decode_sil_caller, the compiled caller of beamSearch with a silence score (tests/test_gpu_beam_sil.py), built by the rules of the
# Makefile beside it -- its compiler, flags and libraries -- through a target of its own:
#   make -C tests/cpp -f decode_sil_caller.mk decode_sil_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/decode_sil_caller: decode_sil_caller.cpp ../../include/fl_compat/flashlight.h ../../include/fl_compat/lexicon.h ../../include/fl_compat/lm.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: decode_sil_caller
decode_sil_caller: $(OUT)/decode_sil_caller
