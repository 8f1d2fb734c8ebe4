# Builds the C++ surface test of the held object against the robot's own segments against the in-tree engine library.
CXX ?= g++
REPO := ../..
OUT ?= build
$(OUT)/held_self: held_self.cpp $(REPO)/include/mppi_amd.hpp $(REPO)/include/mppi_amd.h
	mkdir -p $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(REPO)/include held_self.cpp -L$(REPO)/assistedmanipulation_amd/lib -lmppi_amd \
	  -Wl,-rpath,'$$ORIGIN/../../../assistedmanipulation_amd/lib' -Wl,-rpath,/opt/rocm/lib -o $@
