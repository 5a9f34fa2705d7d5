# Compiler and flags of every HIP translation unit built for the device: the product library (csrc/Makefile) and the
# test-only numerics probe (tests/hip/Makefile) include this one fragment, so the probe is compiled exactly as the kernels.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
# --offload-compress: the gfx950 code objects are stored compressed in the fat binary (14.5 -> ~5 MB; the runtime inflates
# them when the library is loaded)
CXXFLAGS = -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) --offload-compress -Wall -Wno-unused-function -Wno-unused-variable
