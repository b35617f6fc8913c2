#!/usr/bin/env python
"""call_consensus.py -- per-sample consensus sequences from one `merge_midas.py snps` directory, on MI355X.

Drop-in for the reference's scripts/call_consensus.py: same positional argument, option names, defaults and FASTA output.
The matrices are parsed and the consensus bytes formed on the device (midas_amd/analyze/consensus.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    args = cli.consensus_arguments()
    cli.check_consensus_args(args)
    cli.print_copyright()
    cli.print_args(args, 'call_consensus.py')
    from midas_amd.analyze import consensus
    consensus.run_pipeline(args)
