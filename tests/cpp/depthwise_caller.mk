# depthwise_caller, the compiled caller of fl::Conv2D with groups and fl::Swish (tests/test_gpu_depthwise_net.py,
# tests/test_depthwise_host.py), built by the rules of the Makefile beside it -- its compiler, flags and libraries -- through a
# target of its own:
#   make -C tests/cpp -f depthwise_caller.mk depthwise_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/depthwise_caller: depthwise_caller.cpp ../../include/fl_compat/flashlight.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: depthwise_caller
depthwise_caller: $(OUT)/depthwise_caller
