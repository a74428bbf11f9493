# residual_caller, the compiled caller of fl::Residual (tests/test_gpu_residual_caller.py), built by the rules of the Makefile beside
# it -- its compiler, flags and libraries -- through a target of its own:
#   make -C tests/cpp -f residual_caller.mk residual_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/residual_caller: residual_caller.cpp ../../include/fl_compat/flashlight.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: residual_caller
residual_caller: $(OUT)/residual_caller
