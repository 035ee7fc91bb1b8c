# Builds the native pieces in-tree (the .so files travel to the GPU box with gpurun):
#   csvplus_amd/lib/libcsvplus_hip.so   HIP kernels + C ABI (gfx950 only)
#   csvplus_amd/lib/libcph_datagen.so   synthetic table generator (CPU, OpenMP)
#   oracle/_build/liboracle.so          CPU restatement of the reference (test infrastructure)
#   tests/cpp/test_host                 C++ host facade tests (reference-style tests)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function
CC      ?= gcc
CXX     ?= g++

LIBDIR  = csvplus_amd/lib
CSRC    = csvplus_amd/csrc
HIP_SRCS = $(CSRC)/capi.hip $(CSRC)/index_build.hip $(CSRC)/keycodec.hip $(CSRC)/radix_sort.hip $(CSRC)/probe.hip $(CSRC)/chain.hip $(CSRC)/stream_join.hip $(CSRC)/materialize.hip $(CSRC)/json_write.hip $(CSRC)/map_format.hip $(CSRC)/map_switch.hip $(CSRC)/filter.hip $(CSRC)/numparse.hip $(CSRC)/expr_eval.hip $(CSRC)/csv_ingest.hip $(CSRC)/index_ops.hip $(CSRC)/resolve.hip $(CSRC)/aggregate.hip $(CSRC)/join_totals.hip $(CSRC)/order.hip $(CSRC)/dist.hip $(CSRC)/calibrate.hip $(CSRC)/small_build.hip $(CSRC)/host_encode.hip $(CSRC)/window_sort.hip $(CSRC)/counted_sort.hip
HIP_OBJS = $(patsubst $(CSRC)/%.hip,$(LIBDIR)/obj/%.o,$(HIP_SRCS))
HIP_HDRS = $(CSRC)/cph_internal.hpp $(CSRC)/device_utils.hpp $(CSRC)/codec_device.hpp $(CSRC)/probe_device.hpp $(CSRC)/hash_device.hpp $(CSRC)/lds_stage.hpp $(CSRC)/materialize_device.hpp $(CSRC)/map_device.hpp $(CSRC)/map_plan.hpp $(CSRC)/numparse_device.hpp $(CSRC)/floatparse_device.hpp $(CSRC)/pow5_table.inc $(CSRC)/numformat_device.hpp $(CSRC)/shortfmt_device.hpp $(CSRC)/pow10_table.inc $(CSRC)/strpred_device.hpp $(CSRC)/span_device.hpp $(CSRC)/timeparse_device.hpp $(CSRC)/runs_device.hpp $(CSRC)/tile_bitmap.hpp $(CSRC)/num_report.hpp $(CSRC)/order_device.hpp $(CSRC)/csv_lazy_device.hpp $(CSRC)/host_encode_kernels.hpp include/csvplus_hip.h

all: hip datagen oracle host

hip: $(LIBDIR)/libcsvplus_hip.so
datagen: $(LIBDIR)/libcph_datagen.so
oracle: oracle/_build/liboracle.so oracle/_build/libfaithful.so
host: tests/cpp/test_host tests/cpp/test_filter tests/cpp/test_numeric tests/cpp/test_resolve tests/cpp/test_map tests/cpp/test_map_switch tests/cpp/test_totals tests/cpp/test_join_totals tests/cpp/test_map_float tests/cpp/test_expr tests/cpp/test_expr_cond tests/cpp/test_host_encode tests/cpp/test_numformat tests/cpp/test_strpred tests/cpp/test_strpred_facade tests/cpp/test_span tests/cpp/test_span_facade tests/cpp/test_hash_model tests/cpp/test_orderkey tests/cpp/test_order tests/cpp/test_csv_lazy tests/cpp/test_timeparse tests/cpp/test_time tests/cpp/test_floatparse tests/cpp/test_shortfmt tests/cpp/test_map_shortest tests/cpp/test_num_report tests/c/abi_demo tests/c/libnccl_standin.so

$(LIBDIR)/obj/%.o: $(CSRC)/%.hip $(HIP_HDRS)
	@mkdir -p $(LIBDIR)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# Go never fuses a*b+c: the expression kernel is compiled without contraction
$(LIBDIR)/obj/expr_eval.o: HIPFLAGS += -ffp-contract=off

$(LIBDIR)/libcsvplus_hip.so: $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(HIP_OBJS) -ldl -o $@

$(LIBDIR)/libcph_datagen.so: $(CSRC)/datagen.c
	@mkdir -p $(LIBDIR)
	$(CC) -O3 -fopenmp -fPIC -shared -fvisibility=hidden -Wall $< -o $@

oracle/_build/liboracle.so: oracle/csvplus_oracle.c
	@mkdir -p oracle/_build
	$(CC) -O2 -fPIC -shared -fvisibility=hidden -Wall $< -o $@

oracle/_build/libfaithful.so: oracle/faithful.cpp
	@mkdir -p oracle/_build
	$(CXX) -O2 -std=c++17 -fopenmp -fPIC -shared -fvisibility=hidden -Wall $< -o $@

tests/cpp/test_host: tests/cpp/test_host.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_filter: tests/cpp/test_filter.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_numeric: tests/cpp/test_numeric.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_resolve: tests/cpp/test_resolve.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_map: tests/cpp/test_map.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_map_switch: tests/cpp/test_map_switch.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_totals: tests/cpp/test_totals.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_join_totals: tests/cpp/test_join_totals.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_map_float: tests/cpp/test_map_float.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_expr: tests/cpp/test_expr.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

tests/cpp/test_expr_cond: tests/cpp/test_expr_cond.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the Map kernels' float formatter compiled for the host, against glibc's exact "%.*f" (CPU only)
tests/cpp/test_numformat: tests/cpp/test_numformat.cpp $(CSRC)/numformat_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

# the string conditions' per-value routines (the code k_pred_eval runs) compiled for the host, against std::string (CPU only)
tests/cpp/test_strpred: tests/cpp/test_strpred.cpp $(CSRC)/strpred_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

tests/cpp/test_strpred_facade: tests/cpp/test_strpred_facade.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the SPAN piece's operations (the code the Map kernels run per value: trims, affixes, the field search) compiled for the host, against
# Go's definitions restated a byte at a time (CPU only)
tests/cpp/test_span: tests/cpp/test_span.cpp $(CSRC)/span_device.hpp $(CSRC)/strpred_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

tests/cpp/test_span_facade: tests/cpp/test_span_facade.cpp csvplus_amd/host/csvplus.hpp $(CSRC)/span_device.hpp $(CSRC)/strpred_device.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the LazyQuotes separator automaton (the code k_csv_lazy_tile_maps / k_csv_lazy_marks run per chunk) compiled for the host (CPU only)
tests/cpp/test_csv_lazy: tests/cpp/test_csv_lazy.cpp $(CSRC)/csv_lazy_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

# OrderBy's value maps (the code k_order_key runs) compiled for the host, against cmp.Compare (CPU only)
tests/cpp/test_orderkey: tests/cpp/test_orderkey.cpp $(CSRC)/order_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

tests/cpp/test_order: tests/cpp/test_order.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the RFC 3339 routines (the code k_num_parse and the Map kernels run per value) compiled for the host, against gmtime_r / timegm and a
# day counter over years 0000..9999 (CPU only)
tests/cpp/test_timeparse: tests/cpp/test_timeparse.cpp $(CSRC)/timeparse_device.hpp
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

# the Eisel-Lemire float conversion (the code k_num_parse's full float instantiation runs behind Clinger's exact cases) compiled for the
# host, against glibc's strtod (CPU only)
tests/cpp/test_floatparse: tests/cpp/test_floatparse.cpp $(CSRC)/floatparse_device.hpp $(CSRC)/pow5_table.inc
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

# the shortest float formatter (the code the Map kernels run for a FLOAT64_SHORTEST piece) compiled for the host, against std::to_chars
# (CPU only)
tests/cpp/test_shortfmt: tests/cpp/test_shortfmt.cpp $(CSRC)/shortfmt_device.hpp $(CSRC)/pow10_table.inc
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

tests/cpp/test_map_shortest: tests/cpp/test_map_shortest.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the error report's packing (the functions the typed-value kernels and their host code share) compiled for the host (CPU only)
tests/cpp/test_num_report: tests/cpp/test_num_report.cpp $(CSRC)/num_report.hpp include/csvplus_hip.h
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) $< -o $@

tests/cpp/test_time: tests/cpp/test_time.cpp csvplus_amd/host/csvplus.hpp include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -Icsvplus_amd/host $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# the host-side key encoder's loops and worker pool on their own (CPU only)
tests/cpp/test_host_encode: tests/cpp/test_host_encode.cpp $(CSRC)/host_encode_kernels.hpp
	$(CXX) -O2 -std=c++17 -Wall -pthread $< -o $@

# the Join hash table's hash, home sector and probe-sequence step evaluated on the host (CPU only: no HIP call)
tests/cpp/test_hash_model: tests/cpp/test_hash_model.hip $(HIP_HDRS)
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wall -Wno-unused-function $< -o $@

tests/c/abi_demo: tests/c/abi_demo.c include/csvplus_hip.h $(LIBDIR)/libcsvplus_hip.so
	$(CC) -O2 -std=c99 -Wall -Wextra -Iinclude $< -L$(LIBDIR) -lcsvplus_hip -Wl,-rpath,'$$ORIGIN/../../csvplus_amd/lib' -o $@

# NCCL's entry points for thread ranks sharing one GPU (test infrastructure: the RCCL transport of csrc/dist.hip with 2 and 3 ranks)
tests/c/libnccl_standin.so: tests/c/nccl_standin.cpp
	$(HIPCC) -O2 -std=c++17 -fPIC -shared $< -o $@

# ---- sanitizer builds (CPU side only: the checker, the data generator, the host facade's own code) ----------
# tests/test_asan.py runs them; findings abort the run.  The device side has its own canaries: cph_ctx_set_option
# "pool_guard" (tools/gpu_guard.sh runs the whole GPU suite under it).
SAN = -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1
asan: oracle/_build/oracle_fuzz_asan oracle/_build/datagen_asan oracle/_build/timeparse_asan oracle/_build/floatparse_asan oracle/_build/shortfmt_asan oracle/_build/span_asan

# the same stand-alone program as tests/cpp/test_timeparse, under the sanitizers (run it on a CPU machine)
oracle/_build/timeparse_asan: tests/cpp/test_timeparse.cpp $(CSRC)/timeparse_device.hpp
	@mkdir -p oracle/_build
	$(CXX) $(SAN) -std=c++17 -Wall -I$(CSRC) tests/cpp/test_timeparse.cpp -o $@

# the same stand-alone program as tests/cpp/test_floatparse, under the sanitizers (run it on a CPU machine)
oracle/_build/floatparse_asan: tests/cpp/test_floatparse.cpp $(CSRC)/floatparse_device.hpp $(CSRC)/pow5_table.inc
	@mkdir -p oracle/_build
	$(CXX) $(SAN) -std=c++17 -Wall -I$(CSRC) tests/cpp/test_floatparse.cpp -o $@

# the same stand-alone program as tests/cpp/test_shortfmt, under the sanitizers (run it on a CPU machine)
oracle/_build/shortfmt_asan: tests/cpp/test_shortfmt.cpp $(CSRC)/shortfmt_device.hpp $(CSRC)/pow10_table.inc
	@mkdir -p oracle/_build
	$(CXX) $(SAN) -std=c++17 -Wall -I$(CSRC) tests/cpp/test_shortfmt.cpp -o $@

# the same stand-alone program as tests/cpp/test_span, under the sanitizers (run it on a CPU machine)
oracle/_build/span_asan: tests/cpp/test_span.cpp $(CSRC)/span_device.hpp $(CSRC)/strpred_device.hpp
	@mkdir -p oracle/_build
	$(CXX) $(SAN) -std=c++17 -Wall -I$(CSRC) tests/cpp/test_span.cpp -o $@

oracle/_build/oracle_fuzz_asan: tests/c/oracle_fuzz.c oracle/csvplus_oracle.c
	@mkdir -p oracle/_build
	$(CC) $(SAN) -Wall tests/c/oracle_fuzz.c -o $@

oracle/_build/datagen_asan: tests/c/datagen_check.c $(CSRC)/datagen.c
	@mkdir -p oracle/_build
	$(CC) $(SAN) -fopenmp -Wall tests/c/datagen_check.c -o $@

clean:
	rm -rf $(LIBDIR) oracle/_build tests/cpp/test_host tests/cpp/test_filter tests/cpp/test_numeric tests/cpp/test_resolve tests/cpp/test_map tests/cpp/test_map_switch tests/cpp/test_totals tests/cpp/test_join_totals tests/cpp/test_map_float tests/cpp/test_expr tests/cpp/test_expr_cond tests/cpp/test_numformat tests/cpp/test_strpred tests/cpp/test_strpred_facade tests/cpp/test_span tests/cpp/test_span_facade tests/cpp/test_host_encode tests/cpp/test_hash_model tests/cpp/test_orderkey tests/cpp/test_order tests/cpp/test_csv_lazy tests/cpp/test_timeparse tests/cpp/test_time tests/cpp/test_floatparse tests/cpp/test_shortfmt tests/cpp/test_map_shortest tests/cpp/test_num_report tests/c/abi_demo tests/c/libnccl_standin.so

.PHONY: all hip datagen oracle host asan clean
