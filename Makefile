# Convenience targets; the real build is snappy_amd/csrc/Makefile (hipcc, gfx950) and oracle/Makefile (gcc).
all:
	$(MAKE) -C snappy_amd/csrc
	$(MAKE) -C oracle

test: all          # CPU suite: oracle vs golden vectors, host logic, ABI surface, lane simulator, gloo sharding
	python -m pytest tests -x -q -m "not gpu"

test-gpu: all      # needs an MI355X: bit-exact parity through the C ABI
	python -m pytest tests -x -q -m gpu

bench: all         # the headline alone: the timed end-to-end pass
	python bench.py

bench-full: all    # the headline, then the roofline pass, parity vs the oracle, CPU baselines, the other legs and configs
	python bench.py --full

clean:
	$(MAKE) -C snappy_amd/csrc clean
	$(MAKE) -C oracle clean

.PHONY: all test test-gpu bench bench-full clean
