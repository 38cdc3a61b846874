# The build of one family's host simulation -- TEST ONLY.  tests/hostsim_<family>/Makefile sets
#   NAME    : the family; sim_$(NAME).cpp becomes liblce_hostsim_$(NAME).so
#   HEADERS : the kernel headers of csrc/ whose device part the simulation compiles
#   FLAGS   : the family's language level, optimisation and warning flags
#   DEPS    : (optional) further headers of csrc/ the simulation reads in place
# and includes this file.  The real kernel bodies are compiled against the suite's host replacement of the device intrinsics
# (lce_device_intrinsics.h, beside this file) and run lane by lane as fibers (sim_harness.h).  The kernel headers name
# "lce_device_intrinsics.h" in quotes, which finds the file beside them first: build/ holds copies of the kernel headers beside a
# copy of the host replacement (build products, never committed).
CXX ?= g++
CSRC := ../../compute-engine_amd/csrc
HOSTSIM := ../hostsim
TARGET := liblce_hostsim_$(NAME).so
GEN := build
all: $(TARGET)
$(GEN)/.stamp: $(HEADERS) $(HOSTSIM)/lce_device_intrinsics.h
	mkdir -p $(GEN)
	cp $(HEADERS) $(HOSTSIM)/lce_device_intrinsics.h $(GEN)/
	touch $@
$(TARGET): sim_$(NAME).cpp $(GEN)/.stamp $(HOSTSIM)/sim_harness.h $(CSRC)/lce_kernel_args.h $(CSRC)/lce_kernels_common.h $(DEPS)
	$(CXX) $(FLAGS) -fPIC -shared -fno-strict-aliasing -I$(GEN) -I$(CSRC) -I$(HOSTSIM) -o $@ sim_$(NAME).cpp
clean:
	rm -rf $(TARGET) $(GEN)
.PHONY: all clean
