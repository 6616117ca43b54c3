"""Shared by test_value_hist.py and test_value_hist_host.py: the statistics table of `meryl statistics` written out by hand for the
tiny database of test_db_eval_host.tiny_db, and the text of a histogram."""
import numpy as np

# tiny_db(path, 21): four 21-mers with the values 2, 7, 2, 7.  Histogram: 2 -> 2, 7 -> 2; no k-mer with value 1; 4 distinct; 18 in all;
# 4^21 = 4398046511104 possible 21-mers, 4398046511100 of them missing.  Rows (src/meryl/merylOp-histogram.C:87-92, "%9 %12 %12.4f
# %12.4f %12.6f"): cumulative distinct 2/4 and 4/4, cumulative total 4/18 = 0.2222 and 18/18, presence 2/18 and 7/18 in millionths.
TINY_K21_STATISTICS = (
    "Number of 21-mers that are:\n"
    "  unique                      0  (exactly one instance of the kmer is in the input)\n"
    "  distinct                    4  (non-redundant kmer sequences in the input)\n"
    "  present                    18  (...)\n"
    "  missing         4398046511100  (non-redundant kmer sequences not in the input)\n"
    "\n"
    "             number of   cumulative   cumulative     presence\n"
    "              distinct     fraction     fraction   in dataset\n"
    "frequency        kmers     distinct        total       (1e-6)\n"
    "--------- ------------ ------------ ------------ ------------\n"
    "        2            2       0.5000       0.2222 111111.111111\n"
    "        7            2       1.0000       1.0000 388888.888889\n"
)

# k = 32: nUniverse = (2^64 - 1) + 1 wraps to 0 in uint64, so `missing` is 0 - 5 modulo 2^64
K32_STATISTICS = (
    "Number of 32-mers that are:\n"
    "  unique                      3  (exactly one instance of the kmer is in the input)\n"
    "  distinct                    5  (non-redundant kmer sequences in the input)\n"
    "  present                    11  (...)\n"
    "  missing  18446744073709551611  (non-redundant kmer sequences not in the input)\n"
    "\n"
    "             number of   cumulative   cumulative     presence\n"
    "              distinct     fraction     fraction   in dataset\n"
    "frequency        kmers     distinct        total       (1e-6)\n"
    "--------- ------------ ------------ ------------ ------------\n"
    "        1            3       0.6000       0.2727 90909.090909\n"
    "        4            2       1.0000       1.0000 363636.363636\n"
)


def unique_counts(values):
    """the oracle: numpy.unique of the values as uint64"""
    v, o = np.unique(np.asarray(values).astype(np.uint64), return_counts=True)
    return v.astype(np.uint64), o.astype(np.uint64)


def histogram_text(values, occurrences):
    """value <TAB> occurrences per line (src/meryl/merylOp-histogram.C:39-42)"""
    return "".join("%d\t%d\n" % (int(v), int(o)) for v, o in zip(values, occurrences))
