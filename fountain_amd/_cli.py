"""What the package's command lines share: how a file gets its name beside another, and how a command line is refused."""
import sys


def beside(name, suffix):
    """out.exr, "_x.exr" -> out_x.exr: `suffix` in place of an .exr at the end, or after a name that has none."""
    return (name[:-4] if name.endswith(".exr") else name) + suffix


def refuse(msg):
    """Says why the command line is refused; returns the exit code for that."""
    print("error: %s" % msg, file=sys.stderr)
    return 2
