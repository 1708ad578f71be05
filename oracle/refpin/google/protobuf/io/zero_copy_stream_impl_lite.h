// TEST INFRASTRUCTURE ONLY: found through -I where the reference includes
// protobuf's header of this name; StringOutputStream is in standins.hh.
#include "standins.hh"
