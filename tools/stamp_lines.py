"""Prefix every line of stdin with the host seconds since this filter started, optionally a label
first: the epoch lines of an entry point with the time they were printed at (the program has to run
unbuffered).  Usage: python -u another_neural_net.py ... | python -u tools/stamp_lines.py [label]"""
import sys
import time

label = sys.argv[1] + " " if len(sys.argv) > 1 else ""
t0 = time.perf_counter()
for line in sys.stdin:
    sys.stdout.write("%s%9.4f  %s" % (label, time.perf_counter() - t0, line))
    sys.stdout.flush()
