# oracle/hip_host.mk -- builds libray_hip.so: the reference's HOST-SIDE scene code + RendererHIP/SceneHIP + the C view.
#
#     make -f hip_host.mk REF=<reference tree>        (from oracle/; the default target of ./Makefile runs it)
#
# This is the drop-in as a shared library: what you get when RendererHIP.cpp is added to the reference tree with
# every other backend disabled.  The reference translation units are compiled where they lie under $(REF)
# (nothing is copied); only the scene-side ones are needed -- no CPU renderer (CoreRef/ShadeRef's Renderer*
# instantiations) is linked, so this library has no CPU rendering path at all.
# Links against ../ray_amd/csrc/_build/librayhip.so (the HIP kernels behind the C ABI).
#
# It compiles reference sources, so it lands next to the oracle in _ref/ (git-ignored, travels with the tree to a machine
# without the reference): _ref/hip/libray_hip.so.  Objects and generated headers stay in _build/hip/ (not needed at run time).
# This file builds the product's host side, not the checker: the rule of ./Makefile (nothing under ray_amd/ loads
# libray_ref.so) is untouched.

REF      ?= /root/reference
OUT      := _ref/hip
TMP      := _build/hip
GEN      := $(TMP)/gen
OBJ      := $(TMP)/obj
HOST     := ../ray_amd/host
CXX      ?= g++
CXXFLAGS := -O3 -DNDEBUG -std=c++17 -msse2 -mno-avx -fno-strict-aliasing -fPIC -w \
            -I$(GEN) -I$(GEN)/internal -I$(REF) -I$(REF)/internal

# host-side scene code of the reference: storage, BVH build, light tree, textures, sky bake helpers; UNetFilter: the
# denoiser's weight tables and their layout function (RendererHIP::InitUNetFilter hands them to rayhip_unet_init)
INTERNAL := AtmosphereRef BVHSplit CDFUtils Core CoreRef FreelistAlloc SamplingParams SceneCommon SceneCPU \
            TextureParams TextureSplitter TextureStorageCPU TextureUtils TextureUtilsSSE2 Time RadCacheRef TonemapRef UNetFilter
OBJS := $(addprefix $(OBJ)/internal_,$(addsuffix .o,$(INTERNAL))) $(OBJ)/simd_detect.o
FLAGS_internal_TextureUtilsSSE2 := -msse2
# CoreRef.cpp / RadCacheRef.cpp hold the reference's scalar RENDER kernels; the scene code needs four helpers of them
# (TransformPoint / TransformDirection, portable_sincos, Evaluate_EnvQTree).  One section per function + hidden visibility +
# --gc-sections at link time: everything else of those files (IntersectScene, ShadeSurface, ...) is dropped from the product
# binary instead of being exported as dead code.
FLAGS_internal_CoreRef := -ffunction-sections -fdata-sections -fvisibility=hidden
FLAGS_internal_RadCacheRef := -ffunction-sections -fdata-sections -fvisibility=hidden

.PHONY: all clean
all: $(OUT)/libray_hip.so

$(GEN)/.stamp: ../tools/gen_ref_blobs.py
	@mkdir -p $(GEN) $(OBJ) $(OUT)
	python3 ../tools/gen_ref_blobs.py $(REF) $(GEN)
	@touch $@

$(OBJ)/internal_%.o: $(REF)/internal/%.cpp $(GEN)/.stamp
	$(CXX) $(CXXFLAGS) $(FLAGS_internal_$*) -c $< -o $@

$(OBJ)/simd_detect.o: $(REF)/internal/simd/detect.cpp $(GEN)/.stamp
	$(CXX) $(CXXFLAGS) -mxsave -c $< -o $@

$(OBJ)/RendererHIP.o: $(HOST)/RendererHIP.cpp $(HOST)/RendererHIP.h $(HOST)/scene_export.h ../include/rayhip.h $(GEN)/.stamp
	$(CXX) $(CXXFLAGS) -I$(HOST) -c $(HOST)/RendererHIP.cpp -o $@
$(OBJ)/ray_capi.o: $(HOST)/ray_capi.cpp $(HOST)/ray_capi.h $(HOST)/RendererHIP.h $(GEN)/.stamp
	$(CXX) $(CXXFLAGS) -I$(HOST) -DRAY_CAPI_WITH_HIP -c $(HOST)/ray_capi.cpp -o $@

# librayhip.so, linked against below: built by __graft_entry__.build() -- or here, when this recipe runs on a checkout where
# build() has not (the kernels need only hipcc, not the reference tree)
KERNELS := ../ray_amd/csrc/_build/librayhip.so
$(KERNELS):
	cd .. && python3 -c 'import __graft_entry__ as g; g.build_kernels()'

$(OUT)/libray_hip.so: $(OBJS) $(OBJ)/RendererHIP.o $(OBJ)/ray_capi.o | $(KERNELS)
	$(CXX) -shared -Wl,--gc-sections -o $@ $^ -L../ray_amd/csrc/_build -lrayhip -Wl,-rpath,'$$ORIGIN/../../../ray_amd/csrc/_build' -lpthread

clean:
	rm -rf $(OUT) $(TMP)
