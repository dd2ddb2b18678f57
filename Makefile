# Build for MI355X (gfx950).  `make` builds the engine and the oracle (test infrastructure).
# The packed-Shamir kernels are compiled as one object per instantiation family
# (SDA_GEN_PART / SDA_GEN_L = n+1 / k+t+1, SDA_REVEAL_PART = padded point count) so `make -j` builds them in parallel.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function
EXTRA    ?=

CSRC    := sda_amd/csrc
OBJDIR  ?= build/obj
LIB     ?= sda_amd/libsda_engine.so

# share-gen objects, one per (n+1, k+t+1): the n+1 = 81 instantiations dominate the build, so they compile in parallel
GEN_PARTS    := 3_2 9_2 9_4 9_8 27_2 27_4 27_8 27_16 81_2 81_4 81_8 81_16 81_32 81_64
REVEAL_PARTS := 8 16 32 64 96
PLAIN   := combine elementwise chacha codec_decode codec_encode snapshot packed_wide packed_check packed_repair packed_decode draws additive_keyed mask_keyed recipient_job recipient_repair
HOST    := engine engine_dev engine_check hbm engine_codec engine_recipient engine_participant engine_host
OBJS    := $(patsubst %,$(OBJDIR)/%.o,$(PLAIN)) $(patsubst %,$(OBJDIR)/%.o,$(HOST)) \
           $(OBJDIR)/packed_gen.o $(patsubst %,$(OBJDIR)/packed_gen_%.o,$(GEN_PARTS)) \
           $(OBJDIR)/packed_reveal.o $(patsubst %,$(OBJDIR)/packed_reveal_%.o,$(REVEAL_PARTS))
HDRS    := $(CSRC)/packed_common.h $(CSRC)/kernels.h $(CSRC)/reveal_plan.h $(CSRC)/check_plan.h $(CSRC)/repair_plan.h $(CSRC)/decode_plan.h $(CSRC)/decode_tables.h $(CSRC)/decode_core.h $(CSRC)/check_common.h $(CSRC)/check_launch.h $(CSRC)/repair_body.h $(CSRC)/modarith.h $(CSRC)/xcd.h $(CSRC)/draws_common.h $(CSRC)/codec_common.h include/sda_engine.h

all: $(LIB) oracle

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA) -c $< -o $@

$(OBJDIR)/packed_gen_%.o: $(CSRC)/packed_gen.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA) -DSDA_GEN_PART=$(word 1,$(subst _, ,$*)) -DSDA_GEN_L=$(word 2,$(subst _, ,$*)) -c $< -o $@

$(OBJDIR)/packed_reveal_%.o: $(CSRC)/packed_reveal.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA) -DSDA_REVEAL_PART=$* -c $< -o $@

# the host translation units of the C ABI: one object each
$(OBJDIR)/%.o: $(CSRC)/%.cpp $(CSRC)/engine_internal.h $(CSRC)/host_pack.h $(CSRC)/participant_job_plan.h $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA) -x hip -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
