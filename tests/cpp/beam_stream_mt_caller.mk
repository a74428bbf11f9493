# beam_stream_mt_caller, the compiled caller of ManyTokenStreamingDecoder (tests/test_gpu_beam_stream_mt.py), built by the rules of the
# Makefile beside it -- its compiler, flags and libraries -- through a target of its own:
#   make -C tests/cpp -f beam_stream_mt_caller.mk beam_stream_mt_caller [OUT=<dir>]
# OUT (default: this directory) is where the binary goes; the library's absolute path is added to the run path so that it runs from there.
include Makefile
OUT ?= .

$(OUT)/beam_stream_mt_caller: beam_stream_mt_caller.cpp ../../include/fl_compat/flashlight.h ../../include/fl_compat/lm.h $(LIBDIR)/libw2l_hip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS) -Wl,-rpath,$(abspath $(LIBDIR))

.PHONY: beam_stream_mt_caller
beam_stream_mt_caller: $(OUT)/beam_stream_mt_caller
