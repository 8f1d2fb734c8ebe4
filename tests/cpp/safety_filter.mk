# Builds the C++ surface test of the trajectory safety filter against the in-tree engine library.
CXX ?= g++
REPO := ../..
OUT ?= build
$(OUT)/safety_filter: safety_filter.cpp $(REPO)/include/mppi_amd.hpp $(REPO)/include/mppi_amd.h
	mkdir -p $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(REPO)/include safety_filter.cpp -L$(REPO)/assistedmanipulation_amd/lib -lmppi_amd \
	  -Wl,-rpath,'$$ORIGIN/../../../assistedmanipulation_amd/lib' -Wl,-rpath,/opt/rocm/lib -o $@
