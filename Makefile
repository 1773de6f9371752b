# Builds the MI355X (gfx950) engine in-tree:
#   whisper.tflite_amd/lib/libwhisper-tflite.so   C ABI (include/wt_capi.h) + C++ surface
#   whisper.tflite_amd/bin/encdec, bin/minimal    the reference's CLIs, same arguments
#   whisper.tflite_amd/bin/wt-make-assets         synthetic weights / vocab writer
#   oracle/libwt_oracle.so (+ oracle/_ref/)       test infrastructure (see oracle/)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
PKG   := whisper.tflite_amd
SRC   := $(PKG)/csrc
OBJ   := $(PKG)/build
CXXFLAGS := -std=c++17 -O3 -fPIC -Iinclude -I$(SRC) -Wall -Wno-unused-result
HIPFLAGS := $(CXXFLAGS) --offload-arch=$(ARCH) -ffp-contract=fast $(HIPFLAGS_EXTRA)

KERNELS := k_gemm k_gemm_planes k_gemm_bf16 k_misc k_attention k_attention_planes k_decoder k_cross_absorbed k_cross_absorbed_i8 k_beam k_beam_full k_timestamps k_scores k_sample k_align k_suppress k_best_of k_resample k_nucleus k_logits_i8 k_dec_gemm_i8 k_enc_gemm_i8 k_enc_conv_i8
HOSTSRC := engine engine_full decode_results capi capi_debug host_util longform words weights_gen whisper_api tflite_extract resample
OBJS := $(addprefix $(OBJ)/,$(addsuffix .o,$(KERNELS) $(HOSTSRC)))

all: lib apps oracle
lib: $(PKG)/lib/libwhisper-tflite.so
apps: $(PKG)/bin/encdec $(PKG)/bin/minimal $(PKG)/bin/wt-make-assets
oracle:
	$(MAKE) -C oracle

# the attention's softmax runs beside other wavefronts' MFMAs, where packed fp32 instructions (what the SLP vectoriser makes
# of its row sums) cost more than the scalar ones they replace (MI355X_MICROARCH.md, vector-instruction issue costs): 325.8
# against 334.2 us per layer (tools/ab_attn.sh)
$(OBJ)/k_attention_planes.o: HIPFLAGS += -fno-slp-vectorize

# the fixed-point masses of nucleus_cut are products and sums of single floats: no packed fp32 instructions there
$(OBJ)/k_nucleus.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops

# the int8 logits head scales back with two single fp32 products per element: no packed fp32 instructions there either
$(OBJ)/k_logits_i8.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops

# the int8 decoder GEMM likewise; its epilogue is specified product by product and sum by sum, so the
# contract(off) pragma around it has to hold: -ffp-contract=fast fuses whatever the source says
$(OBJ)/k_dec_gemm_i8.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops -ffp-contract=fast-honor-pragmas

# the int8 encoder GEMM and its row quantiser: the same arithmetic, the same flags
$(OBJ)/k_enc_gemm_i8.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops -ffp-contract=fast-honor-pragmas

# the int8 encoder conv stem: the same epilogue arithmetic, the same flags
$(OBJ)/k_enc_conv_i8.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops -ffp-contract=fast-honor-pragmas

$(OBJ)/%.o: $(SRC)/%.hip $(SRC)/kernels.h $(SRC)/ts_rules.h $(SRC)/dec_rows.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/%.o: $(SRC)/%.cpp $(wildcard $(SRC)/*.h) $(wildcard include/*.h)
	@mkdir -p $(OBJ)
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

$(PKG)/lib/libwhisper-tflite.so: $(OBJS)
	@mkdir -p $(PKG)/lib
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS)

$(PKG)/bin/encdec: $(PKG)/app/encdec.cpp $(PKG)/lib/libwhisper-tflite.so
	@mkdir -p $(PKG)/bin
	$(HIPCC) $(CXXFLAGS) -o $@ $< -L$(PKG)/lib -lwhisper-tflite -Wl,-rpath,'$$ORIGIN/../lib'

$(PKG)/bin/minimal: $(PKG)/app/minimal.cpp $(PKG)/lib/libwhisper-tflite.so
	@mkdir -p $(PKG)/bin
	$(HIPCC) $(CXXFLAGS) -o $@ $< -L$(PKG)/lib -lwhisper-tflite -Wl,-rpath,'$$ORIGIN/../lib'

$(PKG)/bin/wt-make-assets: $(PKG)/app/make_assets.cpp $(PKG)/lib/libwhisper-tflite.so
	@mkdir -p $(PKG)/bin
	$(HIPCC) $(CXXFLAGS) -o $@ $< -L$(PKG)/lib -lwhisper-tflite -Wl,-rpath,'$$ORIGIN/../lib'

clean:
	rm -rf $(OBJ) $(PKG)/lib $(PKG)/bin
	$(MAKE) -C oracle clean
.PHONY: all lib apps oracle clean
