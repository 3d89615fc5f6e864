# Top-level build: the gfx950 engine (HIP, C ABI) and the CPU checker under oracle/.
# hipcc cross-compiles for gfx950 without a GPU.  No FP contraction, no fast-math:
# the numerics contract depends on it.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
# EXTRA=-DSCL_DIAGNOSTICS builds the SC-distance kernels' phase ablation / stamps / occupancy overrides in
# (scripts/ablate_k1.sh); the product build has none of them
EXTRA   ?=
CSRC    := scl_slam_amd/csrc
LIBDIR  := scl_slam_amd/lib
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-result -Iinclude -I$(CSRC) $(EXTRA)
SRCS    := $(CSRC)/engine.hip $(CSRC)/ingest_host.hip $(CSRC)/screen_host.hip $(CSRC)/registration.hip $(CSRC)/sc_distance.hip $(CSRC)/ringkey_topk.hip $(CSRC)/make_sc.hip $(CSRC)/icp.hip $(CSRC)/voxel.hip $(CSRC)/sharded_front.hip $(CSRC)/sc_screen.hip $(CSRC)/sc_masked.hip $(CSRC)/sc_matrix.hip $(CSRC)/sc_rank.hip $(CSRC)/messages.hip $(CSRC)/iris.hip $(CSRC)/device_sort.hip $(CSRC)/m2dp.hip $(CSRC)/fpfh.hip $(CSRC)/grsd.hip $(CSRC)/pcm.hip $(CSRC)/pgo.hip $(CSRC)/pgo_condensed.hip $(CSRC)/pgo_marginals.hip $(CSRC)/global_map.hip
OBJS    := $(SRCS:.hip=.o)
# the adapter template the M2DP, FPFH and GRSD adapters derive from, and the batch declarations their C headers share
VP_ADAPTER := include/scl/vector_plugin_hip_descriptor.hpp include/scl_plugin_batch.h

all: $(LIBDIR)/libscl_engine.so oracle tests/cpp/adapter_check tests/cpp/m2dp_adapter_check tests/cpp/fpfh_adapter_check tests/cpp/grsd_adapter_check tests/cpp/plugin_batch_check tests/cpp/plugin_topk_check tests/cpp/iris_batch_check tests/cpp/iris_search_check tests/cpp/sc_search_check tests/cpp/sc_search_robot_check tests/cpp/nn_plan_check tests/cpp/candidate_windows_check tests/cpp/screen_plan_check tests/cpp/ingest_plan_check tests/cpp/grid_limits_check tests/cpp/pgo_graph_check tests/cpp/pgo_condense_plan_check tests/cpp/pgo_marginal_plan_check tests/cpp/global_map_plan_check tests/cpp/libfpfh_checker.so tests/cpp/libgrsd_checker.so tests/cpp/libmock_rccl.so

$(CSRC)/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.hpp) include/scl_engine.h include/scl_m2dp.h include/scl_fpfh.h include/scl_grsd.h include/scl_iris.h include/scl_plugin_batch.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libscl_engine.so: $(OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl

oracle:
	$(MAKE) -C oracle

# C++ host-side adapter (include/scl/scan_context_hip_descriptor.hpp) type-checked and linked
# against the C ABI; runs on the GPU box (tests/test_gpu_adapter.py)
tests/cpp/adapter_check: tests/cpp/adapter_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/scan_context_hip_descriptor.hpp include/scl/lidar_iris_hip_descriptor.hpp $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/adapter_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the M2DP adapter (include/scl/m2dp_hip_descriptor.hpp) against the C ABI; runs on the GPU box (tests/test_gpu_m2dp.py)
tests/cpp/m2dp_adapter_check: tests/cpp/m2dp_adapter_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/m2dp_hip_descriptor.hpp $(VP_ADAPTER) include/scl_m2dp.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/m2dp_adapter_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the FPFH adapter (include/scl/fpfh_hip_descriptor.hpp) against the C ABI; runs on the GPU box (tests/test_gpu_fpfh.py)
tests/cpp/fpfh_adapter_check: tests/cpp/fpfh_adapter_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/fpfh_hip_descriptor.hpp $(VP_ADAPTER) include/scl_fpfh.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/fpfh_adapter_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the GRSD adapter (include/scl/grsd_hip_descriptor.hpp) against the C ABI; runs on the GPU box (tests/test_gpu_grsd.py)
tests/cpp/grsd_adapter_check: tests/cpp/grsd_adapter_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/grsd_hip_descriptor.hpp $(VP_ADAPTER) include/scl_grsd.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/grsd_adapter_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the batch forms of the M2DP, FPFH and GRSD adapters against loops over the virtuals; runs on the GPU box (tests/test_gpu_plugin_batch_adapter.py)
tests/cpp/plugin_batch_check: tests/cpp/plugin_batch_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/m2dp_hip_descriptor.hpp include/scl/fpfh_hip_descriptor.hpp include/scl/grsd_hip_descriptor.hpp $(VP_ADAPTER) include/scl_m2dp.h include/scl_fpfh.h include/scl_grsd.h include/scl_plugin_batch.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/plugin_batch_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the candidate lists of the M2DP, FPFH and GRSD adapters against the C calls; runs on the GPU box (tests/test_gpu_plugin_topk_adapter.py)
tests/cpp/plugin_topk_check: tests/cpp/plugin_topk_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/m2dp_hip_descriptor.hpp include/scl/fpfh_hip_descriptor.hpp include/scl/grsd_hip_descriptor.hpp $(VP_ADAPTER) include/scl_m2dp.h include/scl_fpfh.h include/scl_grsd.h include/scl_plugin_batch.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/plugin_topk_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the batch forms of the LiDAR-Iris adapter against loops over its six virtuals; runs on the GPU box (tests/test_gpu_iris_batch_adapter.py)
tests/cpp/iris_batch_check: tests/cpp/iris_batch_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/lidar_iris_hip_descriptor.hpp include/scl_iris.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/iris_batch_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the exhaustive ranked search of the LiDAR-Iris adapter against the C calls; runs on the GPU box (tests/test_gpu_iris_search_adapter.py)
tests/cpp/iris_search_check: tests/cpp/iris_search_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/lidar_iris_hip_descriptor.hpp include/scl_iris.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/iris_search_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the ranked search of the Scan Context adapter against the C call; runs on the GPU box (tests/test_gpu_sc_search_adapter.py)
tests/cpp/sc_search_check: tests/cpp/sc_search_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/scan_context_hip_descriptor.hpp include/scl_engine.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/sc_search_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

tests/cpp/sc_search_robot_check: tests/cpp/sc_search_robot_check.cpp tests/cpp/pcl_types_for_adapter_check.h include/scl/scan_context_hip_descriptor.hpp include/scl_engine.h $(LIBDIR)/libscl_engine.so
	g++ -std=c++14 -O2 -Wall -Iinclude -Itests/cpp -o $@ tests/cpp/sc_search_robot_check.cpp -L$(LIBDIR) -lscl_engine -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)'

# the plan of the vector plugins' batched search (nn_plan.hpp, host code only) under ASan + UBSan, a program of its own; runs without
# a GPU (tests/test_nn_plan.py)
tests/cpp/nn_plan_check: tests/cpp/nn_plan_check.cpp $(CSRC)/nn_plan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/nn_plan_check.cpp

# the windows of a list of loop candidates and a round's slice of them (candidate_windows.hpp, host code only) under ASan + UBSan, a
# program of its own; runs without a GPU (tests/test_candidate_windows.py)
tests/cpp/candidate_windows_check: tests/cpp/candidate_windows_check.cpp $(CSRC)/candidate_windows.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/candidate_windows_check.cpp

# the launch schedule of a chunk of the screened stream form (screen_plan.hpp, host code only) under ASan + UBSan, a program of its own;
# runs without a GPU (tests/test_screen_plan.py)
tests/cpp/screen_plan_check: tests/cpp/screen_plan_check.cpp $(CSRC)/screen_plan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/screen_plan_check.cpp

# the copy plan of a group of clouds of the points pipeline (ingest_plan.hpp) and the table of the database's arrays (db_arrays.hpp), host
# code only, under ASan + UBSan, a program of its own; runs without a GPU (tests/test_ingest_plan.py)
tests/cpp/ingest_plan_check: tests/cpp/ingest_plan_check.cpp $(CSRC)/ingest_plan.hpp $(CSRC)/db_arrays.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/ingest_plan_check.cpp

# the grid contract (grid_limits.hpp: which num_ring x num_sector scl_create takes, the exact kernels' plans; host code only) under
# ASan + UBSan, a program of its own; runs without a GPU (tests/test_grid_limits.py)
tests/cpp/grid_limits_check: tests/cpp/grid_limits_check.cpp $(CSRC)/grid_limits.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/grid_limits_check.cpp

# the connectivity check and the incidence lists of the pose-graph solve (pgo_graph.hpp, host code only) under ASan + UBSan, a program of
# its own; runs without a GPU (tests/test_pgo_abi.py)
tests/cpp/pgo_graph_check: tests/cpp/pgo_graph_check.cpp $(CSRC)/pgo_graph.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/pgo_graph_check.cpp

# the plan of the condensed direct step (pgo_condense_plan.hpp, host code only) under ASan + UBSan, a program of its own; runs without a
# GPU (tests/test_pgo_condensed_abi.py)
tests/cpp/pgo_condense_plan_check: tests/cpp/pgo_condense_plan_check.cpp $(CSRC)/pgo_condense_plan.hpp $(CSRC)/pgo_graph.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/pgo_condense_plan_check.cpp

# the column groups and the query selection of the many-column solve and the marginals (pgo_marginal_plan.hpp, host code only) under
# ASan + UBSan, a program of its own; runs without a GPU (tests/test_pgo_marginals_abi.py)
tests/cpp/pgo_marginal_plan_check: tests/cpp/pgo_marginal_plan_check.cpp $(CSRC)/pgo_marginal_plan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/pgo_marginal_plan_check.cpp

# the plan of the global voxel map (global_map_plan.hpp, host code only: capacity rule, hash, the diff of a set call, launch groups) under
# ASan + UBSan, a program of its own; runs without a GPU (tests/test_global_map_abi.py)
tests/cpp/global_map_plan_check: tests/cpp/global_map_plan_check.cpp $(CSRC)/global_map_plan.hpp
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -I$(CSRC) -o $@ tests/cpp/global_map_plan_check.cpp

# TEST INFRASTRUCTURE: the FPFH CPU checker (tests/fpfh_checker.py loads it); atan2f from oracle/liboracle.so.  No -march, no
# contraction: every float operation is the one written
tests/cpp/libfpfh_checker.so: tests/cpp/fpfh_checker.c | oracle
	gcc -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -Wall -std=gnu11 -o $@ tests/cpp/fpfh_checker.c -Loracle -loracle -Wl,-rpath,'$$ORIGIN/../../oracle' -lm -lpthread

# TEST INFRASTRUCTURE: the GRSD CPU checker (tests/grsd_checker.py loads it); acosf from tests/cpp/libfpfh_checker.so.  Same flags
tests/cpp/libgrsd_checker.so: tests/cpp/grsd_checker.c tests/cpp/libfpfh_checker.so
	gcc -O2 -ffp-contract=off -fno-fast-math -fPIC -shared -Wall -std=gnu11 -o $@ tests/cpp/grsd_checker.c -Ltests/cpp -lfpfh_checker -Wl,-rpath,'$$ORIGIN' -lm -lpthread

# TEST INFRASTRUCTURE: the stand-in collective the sharded front's G > 1 test loads through SCL_RCCL_LIB (never linked into the product)
tests/cpp/libmock_rccl.so: tests/cpp/mock_rccl.cpp
	$(HIPCC) -x hip --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -shared -o $@ $<

# Sanitizers + fuzzing over everything that builds without a GPU (log: profiles/rNN/sanitize.txt):
#   1. the CPU checker under ASan + UBSan: the whole `-m "not gpu"` suite against oracle/liboracle_asan.so
#   2. the checker's worker pool under TSan (oracle/tools/tsan_pool_driver)
#   3. libFuzzer + ASan + UBSan over the host-only parsers of untrusted bytes: the ROS wire decoders (messages.hip, compiled as host
#      C++) and the database dump parser (db_file.hpp) -- FUZZ_SECONDS (600) of mutation from tests/cpp/fuzz_seeds.py's corpus
CLANGXX ?= /opt/rocm/lib/llvm/bin/clang++
FUZZ_SECONDS ?= 600
SAN_LOG ?= profiles/r05/sanitize.txt
# (-asan-globals=0: ROCm's clang registers the binary's instrumented globals twice and ASan reports every string literal as an ODR
#  violation before main() runs; heap, stack and UB checks -- what a parser of untrusted bytes can get wrong -- are unaffected)
tests/cpp/fuzz_host: tests/cpp/fuzz_host.cpp $(CSRC)/messages.hip $(CSRC)/db_file.hpp include/scl_messages.h include/scl_engine.h
	$(CLANGXX) -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=fuzzer,address,undefined -fno-sanitize-recover=undefined -mllvm -asan-globals=0 \
	    -Iinclude -I$(CSRC) -o $@ tests/cpp/fuzz_host.cpp

sanitize: tests/cpp/fuzz_host
	$(MAKE) -C oracle liboracle_asan.so tools/tsan_pool_driver
	@mkdir -p $(dir $(SAN_LOG)) /tmp/scl_fuzz_corpus
	@echo "== make sanitize: $$(date -u +%Y-%m-%dT%H:%MZ), $$(gcc --version | head -1), $$($(CLANGXX) --version | head -1)" > $(SAN_LOG)
	@echo "== 1. CPU tests against oracle/liboracle_asan.so (-fsanitize=address,undefined, libasan preloaded into python)" >> $(SAN_LOG)
	SCL_ORACLE_LIB=oracle/liboracle_asan.so LD_PRELOAD=$$(gcc -print-file-name=libasan.so):$$(gcc -print-file-name=libubsan.so) \
	    ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	    python -m pytest tests -x -q -m "not gpu" -p no:cacheprovider > /tmp/scl_san_tests.log 2>&1; \
	    grep -E "runtime error|ERROR: AddressSanitizer|SUMMARY" /tmp/scl_san_tests.log | head -5 >> $(SAN_LOG); tail -2 /tmp/scl_san_tests.log >> $(SAN_LOG)
	@echo "== 2. worker pool under ThreadSanitizer (oracle/tools/tsan_pool_driver)" >> $(SAN_LOG)
	TSAN_OPTIONS=halt_on_error=1 oracle/tools/tsan_pool_driver >> $(SAN_LOG) 2>&1
	@echo "== 3. libFuzzer + ASan + UBSan: wire decoders (messages.hip) and dump parser (db_file.hpp), $(FUZZ_SECONDS) s" >> $(SAN_LOG)
	python tests/cpp/fuzz_seeds.py /tmp/scl_fuzz_corpus
	tests/cpp/fuzz_host -max_total_time=$(FUZZ_SECONDS) -max_len=4096 -print_final_stats=1 /tmp/scl_fuzz_corpus 2>&1 | grep -E "stat::|ERROR|SUMMARY|Done|cov:" | tail -12 >> $(SAN_LOG)
	@echo "== done: no finding above means none was reported (every tool stops at its first)" >> $(SAN_LOG)
	@cat $(SAN_LOG)

clean:
	rm -f $(OBJS) $(LIBDIR)/libscl_engine.so tests/cpp/adapter_check tests/cpp/m2dp_adapter_check tests/cpp/fpfh_adapter_check tests/cpp/grsd_adapter_check tests/cpp/plugin_batch_check tests/cpp/plugin_topk_check tests/cpp/iris_batch_check tests/cpp/iris_search_check tests/cpp/sc_search_check tests/cpp/sc_search_robot_check tests/cpp/nn_plan_check tests/cpp/candidate_windows_check tests/cpp/screen_plan_check tests/cpp/ingest_plan_check tests/cpp/grid_limits_check tests/cpp/pgo_graph_check tests/cpp/pgo_condense_plan_check tests/cpp/pgo_marginal_plan_check tests/cpp/global_map_plan_check tests/cpp/libfpfh_checker.so tests/cpp/libgrsd_checker.so tests/cpp/libmock_rccl.so
	$(MAKE) -C oracle clean

.PHONY: all oracle clean sanitize
