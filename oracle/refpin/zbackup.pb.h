// TEST INFRASTRUCTURE ONLY: found through -I where the reference includes its
// generated "zbackup.pb.h"; the message classes are in standins.hh.
#include "standins.hh"
