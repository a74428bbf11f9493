# rnn_caller, the compiled caller of fl::RNN (tests/test_gpu_rnn.py),
# built by the rules of the Makefile beside it -- its compiler, flags and libraries -- through a
# target of its own:
#   make -C tests/cpp -f rnn_caller.mk rnn_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/rnn_caller: rnn_caller.cpp ../../include/fl_compat/flashlight.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: rnn_caller
rnn_caller: $(OUT)/rnn_caller
