#!/usr/bin/env python
"""strain_tracking.py -- marker alleles of strains and their sharing between samples, from one `merge_midas.py snps`
directory, on MI355X.

Drop-in for the reference's scripts/strain_tracking.py: the commands id_markers and track_markers with its option names,
defaults and output tables.  The matrices are parsed, called and paired on the device (midas_amd/analyze/strains.py).
"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

if __name__ == '__main__':
    from midas_amd.analyze import cli
    program = cli.strain_program()
    args = cli.id_markers_arguments() if program == 'id_markers' else cli.track_markers_arguments()
    cli.print_copyright()
    from midas_amd.analyze import strains
    if program == 'id_markers':
        strains.id_markers(args)
    else:
        strains.track_markers(args)
