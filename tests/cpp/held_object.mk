# Builds the C++ surface test of obstacle avoidance with a held object against the in-tree engine library.
CXX ?= g++
REPO := ../..
OUT ?= build
$(OUT)/held_object: held_object.cpp $(REPO)/include/mppi_amd.hpp $(REPO)/include/mppi_amd.h
	mkdir -p $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -I$(REPO)/include held_object.cpp -L$(REPO)/assistedmanipulation_amd/lib -lmppi_amd \
	  -Wl,-rpath,'$$ORIGIN/../../../assistedmanipulation_amd/lib' -Wl,-rpath,/opt/rocm/lib -o $@
