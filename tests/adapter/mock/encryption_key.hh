// TEST INFRASTRUCTURE: stand-in for zbackup's EncryptionKey with the members
// integration/gpu_backup_creator.hh uses (hasKey, getKey, KeySize).  The real
// class derives the key from the repository password; this one is handed 16 bytes.
#ifndef MOCK_ENCRYPTION_KEY_HH
#define MOCK_ENCRYPTION_KEY_HH

#include <string.h>

class EncryptionKey
{
  bool isSet;
  char bytes[ 16 ];

public:
  unsigned const static KeySize = 16;

  EncryptionKey(): isSet( false ) { memset( bytes, 0, sizeof( bytes ) ); }
  explicit EncryptionKey( void const * key16 ): isSet( true ) { memcpy( bytes, key16, sizeof( bytes ) ); }

  bool hasKey() const { return isSet; }
  void const * getKey() const { return bytes; }
};

#endif
